#!/usr/bin/env python3
"""Wall and device time of hnet_sessions_keyframe_relocalise next to a track in the same run, on a GPU:
  python tools/photo_search_bench.py [--cameras 8 64] [--ticks 40] [--warmup 5] [--levels 4] [--iterations 6] [--capacity 3]
Per K cameras one sessions object with a keyframe map.  Every tick pushes the next frame of an out-and-back path (4 seeds, cycled) to all K sessions, then
times, with the same alignment options,
  track       hnet_sessions_keyframe_track: with max_age = 1 for the first `capacity` ticks (every tick re-keys: the map is full), then with
              auto_rekey = 0, so that the held keyframe stays the frame of tick capacity - 1 and every timed alignment spans up to 20 px like a real one
              (with a re-key at every tick the held keyframe would be the current frame itself, which the search finds at once),
  relocalise  hnet_sessions_keyframe_relocalise of the same sessions after the track (max_closure_px 1e-6: every candidate is searched, the alignment
              runs against the pick and the call is REJECTED, so that the next tick's track sees the state the track left).  The pick is the best
              match among the held keyframe and the stored ones, i.e. the nearest: 0 - 10 px from the current frame where the track's keyframe is up to
              20 px away, so the relocalise's alignment is the shorter of the two,
  search      hnet_sessions_photo_search of the same sessions' (prev, curr) pairs: one pair per session, wall only (the call has no device timer).
Wall: the call; device: hnet_sessions_last_keyframe_device_ms.  Medians over --ticks ticks after --warmup.  A relocalise and a track run the same
alignment sequence at the same levels, so relocalise - track (device) is the thumbnails, the search of every candidate (held keyframe + capacity - 1
stored ones) and the pick; the alignment's share is the track's device time less its four small launches."""
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
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--capacity", type=int, default=3)
    a = ap.parse_args()
    import keyframe_util as K
    from cuahn_vio_amd import _capi, weights
    from cuahn_vio_amd.homography_net import HnetEngine, HnetSessions
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    seqs = [K.sequence("out-and-back", seed) for seed in (1, 2, 5, 11)]
    for n in a.cameras:
        e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=n)
        s = HnetSessions(e, n)
        s.enable_keyframes()
        s.enable_keyframe_map(a.capacity)
        ids = np.arange(n, dtype=np.int32)
        kw = dict(levels=a.levels, max_iterations=a.iterations)
        rows, seen, searched = [], 0, 0
        for t in range(a.warmup + a.ticks + 1):
            f = t % 8                                                  # frame 8 of the path is frame 0's pose: the path repeats
            frames = np.stack([seqs[i % 4][0][f] for i in range(n)])
            steps = np.stack([seqs[i % 4][2][f if f else 8] for i in range(n)])
            s.push(ids, frames)
            t0 = time.perf_counter()
            s.keyframe_track(ids, steps, **(dict(max_age=1) if t < a.capacity else dict(auto_rekey=0)), **kw)
            row = [(time.perf_counter() - t0) * 1e3, s.last_keyframe_device_ms()]
            t0 = time.perf_counter()
            rl = s.keyframe_relocalise(ids, max_closure_px=1e-6, **kw)
            row += [(time.perf_counter() - t0) * 1e3, s.last_keyframe_device_ms()]
            if t == 0:
                continue
            t0 = time.perf_counter()
            s.photo_search(ids)
            row += [(time.perf_counter() - t0) * 1e3]
            seen |= int(np.bitwise_or.reduce(rl["rv"]["flags"]))
            searched = int(rl["n_searched"].max())
            rows.append(row)
        r = np.median(np.array(rows[a.warmup:]), axis=0)
        print(f"K = {n:3d}, levels={a.levels} K_trials={a.iterations} capacity={a.capacity}: track wall {r[0]:.4f} ms, device {r[1]:.4f} ms | relocalise wall {r[2]:.4f} ms, "
              f"device {r[3]:.4f} ms | relocalise - track (thumbnails, search of {searched} candidates per session, pick): wall {r[2] - r[0]:+.4f} ms, device "
              f"{r[3] - r[1]:+.4f} ms | search of one pair per session, whole call: wall {r[4]:.4f} ms (relocalise flags seen after the first tick: {seen}; "
              f"{_capi.RL_CLOSURE_ABOVE_MAX} = rejected after the alignment, {_capi.RL_NO_CANDIDATE} = nothing found)", flush=True)
        s.close()
        e.close()


if __name__ == "__main__":
    main()
