#!/usr/bin/env python3
"""Wall and device time of one hnet_sessions_keyframe_track against hnet_sessions_photo_align_robust on the consecutive pair, on a GPU:
  python tools/keyframe_bench.py [--cameras 8 64] [--ticks 40] [--warmup 5] [--levels 3] [--iterations 6]
Per K cameras: every tick pushes the next frame of an out-and-back path (4 seeds, cycled) to all K sessions, then times, with the same options,
  track   hnet_sessions_keyframe_track from the noisy step (wall: the call; device: hnet_sessions_last_keyframe_device_ms),
  pair    hnet_sessions_photo_align_robust on (prev, curr) from the same step (wall: the call; device: hnet_last_photo_align_device_ms).
Medians over --ticks ticks after --warmup.  The difference is the price of the four launches around the alignment and of the larger download; the
alignments themselves differ too (the keyframe is up to 20 px away, the previous frame 5)."""
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
    a = ap.parse_args()
    import keyframe_util as K
    from cuahn_vio_amd import weights
    from cuahn_vio_amd.homography_net import HnetEngine, HnetSessions
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    seqs = [K.sequence("out-and-back", seed) for seed in (1, 2, 5, 11)]
    for n in a.cameras:
        e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=n)
        s = HnetSessions(e, n)
        s.enable_keyframes()
        ids = np.arange(n, dtype=np.int32)
        rows, flags = [], 0
        for t in range(a.warmup + a.ticks + 1):
            f = t % 8                                                  # frame 8 of the path is frame 0's pose: the path repeats
            frames = np.stack([seqs[i % 4][0][f] for i in range(n)])
            steps = np.stack([seqs[i % 4][2][f if f else 8] for i in range(n)])
            s.push(ids, frames)
            t0 = time.perf_counter()
            tr = s.keyframe_track(ids, steps, levels=a.levels, max_iterations=a.iterations)
            t1 = time.perf_counter()
            if t == 0:
                continue
            flags |= int(np.bitwise_or.reduce(tr["flags"]))
            t2 = time.perf_counter()
            s.photo_align_robust(ids, steps, levels=a.levels, max_iterations=a.iterations)
            t3 = time.perf_counter()
            rows.append(((t1 - t0) * 1e3, s.last_keyframe_device_ms(), (t3 - t2) * 1e3, e.last_photo_align_device_ms()))
        r = np.median(np.array(rows[a.warmup:]), axis=0)
        print(f"K = {n:3d}, levels={a.levels} K_trials={a.iterations}: track wall {r[0]:.4f} ms, device {r[1]:.4f} ms | pair wall {r[2]:.4f} ms, device {r[3]:.4f} ms | "
              f"track - pair: wall {r[0] - r[2]:+.4f} ms, device {r[1] - r[3]:+.4f} ms (flags seen after the first tick: {flags})", flush=True)
        s.close()
        e.close()


if __name__ == "__main__":
    main()
