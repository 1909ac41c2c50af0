#!/usr/bin/env python3
"""Wall and device time of hnet_sessions_photo_search_oriented and hnet_sessions_keyframe_relocalise_oriented next to the plain calls in the same run
(DESIGN 7s), on a GPU:
  python tools/photo_search_oriented_bench.py [--cameras 8 64] [--ticks 40] [--warmup 5] [--levels 4] [--iterations 6] [--capacity 3]
The setting is tools/photo_search_bench.py's: per K cameras one sessions object with a keyframe map, every tick pushes the next frame of an out-and-back
path (4 seeds, cycled) to all K sessions and tracks it (max_age = 1 for the first `capacity` ticks, then auto_rekey = 0).  Then, per tick and with the
same options,
  search            hnet_sessions_photo_search of the sessions' (prev, curr) pairs, wall (the call has no device timer),
  relocalise        hnet_sessions_keyframe_relocalise, wall and device (max_closure_px 1e-6: every candidate is searched, the alignment runs against the
                    pick and the call is REJECTED, so that the next tick's track sees the state the track left),
  and per table of 1 (the identity), 13 (+/- 36 degrees in steps of 6: a search bounded by a gyro) and 60 entries (the default)
  search, oriented      hnet_sessions_photo_search_oriented, wall,
  relocalise, oriented  hnet_sessions_keyframe_relocalise_oriented, wall and device, rejected in the same way.
Medians over --ticks ticks after --warmup.  Both relocalises run the same alignment from the same start here (the path is not turned: the identity entry
wins), so oriented - plain (device) is what the table costs: (entries - 1) more searches per candidate and the winner's launch."""
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
    tables = [_capi.photo_search_yaw_table(0.0, 6.0, 1), _capi.photo_search_yaw_table(-36.0, 6.0, 13), _capi.photo_search_yaw_table()]
    for n in a.cameras:
        e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=n)
        s = HnetSessions(e, n)
        s.enable_keyframes()
        s.enable_keyframe_map(a.capacity)
        ids = np.arange(n, dtype=np.int32)
        kw = dict(levels=a.levels, max_iterations=a.iterations)
        rows, searched, winners = [], 0, set()

        def timed(f):
            t0 = time.perf_counter()
            out = f()
            return out, (time.perf_counter() - t0) * 1e3
        for t in range(a.warmup + a.ticks + 1):
            f = t % 8                                                  # frame 8 of the path is frame 0's pose: the path repeats
            frames = np.stack([seqs[i % 4][0][f] for i in range(n)])
            steps = np.stack([seqs[i % 4][2][f if f else 8] for i in range(n)])
            s.push(ids, frames)
            s.keyframe_track(ids, steps, **(dict(max_age=1) if t < a.capacity else dict(auto_rekey=0)), **kw)
            if t == 0:
                continue
            _, w = timed(lambda: s.photo_search(ids))
            row = [w]
            rl, w = timed(lambda: s.keyframe_relocalise(ids, max_closure_px=1e-6, **kw))
            row += [w, s.last_keyframe_device_ms()]
            searched = int(rl["n_searched"].max())
            for tab in tables:
                _, w = timed(lambda: s.photo_search_oriented(ids, hyps=tab))
                row += [w]
                ro, w = timed(lambda: s.keyframe_relocalise_oriented(ids, hyps=tab, max_closure_px=1e-6, **kw))
                row += [w, s.last_keyframe_device_ms()]
                assert not (ro["rv"]["flags"] & (_capi.RL_ATTACHED | _capi.RL_RETRACKED)).any()
                winners |= set(int(h) - int(np.argmax(tab["b"][:, 0])) for h in ro["search"]["hyp"] if h >= 0)
            rows.append(row)
        r = np.median(np.array(rows[a.warmup:]), axis=0)
        print(f"K = {n:3d}, levels={a.levels} K_trials={a.iterations} capacity={a.capacity}, {searched} candidates per session: plain search wall {r[0]:.4f} ms | plain "
              f"relocalise wall {r[1]:.4f} ms, device {r[2]:.4f} ms", flush=True)
        for i, tab in enumerate(tables):
            sw, rw, rd = r[3 + 3 * i: 6 + 3 * i]
            print(f"    {len(tab):2d} entries: oriented search wall {sw:.4f} ms ({sw - r[0]:+.4f}) | oriented relocalise wall {rw:.4f} ms, device {rd:.4f} ms "
                  f"(device - plain {rd - r[2]:+.4f} ms, {(rd - r[2]) / (searched * len(tab)) * 1e3:.3f} us per entry and candidate of a call of {n})", flush=True)
        print(f"    winning entries, as steps from the identity: {sorted(winners)}", flush=True)
        s.close()
        e.close()


if __name__ == "__main__":
    main()
