#!/usr/bin/env python3
"""Wall and device time of hnet_sessions_keyframe_track_recover next to hnet_sessions_keyframe_track and to the two-call alternative, on a GPU:
  python tools/keyframe_recover_bench.py [--cameras 8 64] [--ticks 40] [--warmup 5] [--levels 4] [--iterations 6] [--capacity 3] [--parent DIR] [--rounds 3]
The setting is tools/photo_search_oriented_bench.py's: per K cameras one sessions object with a keyframe map of `capacity` slots, every tick pushes the next
frame of an out-and-back path (4 seeds, cycled) to all K sessions.  Medians over --ticks ticks after --warmup, wall and device (event) time.
  (i)   track            hnet_sessions_keyframe_track (max_age = 1 for the first `capacity` ticks, then auto_rekey = 0), in a process of its own.  With
                         --parent DIR (a built checkout of the parent commit) the same measurement runs on that tree's package and library, the two in turn
                         --rounds times: a median of this tree above the parent's largest by more than the parent's own spread is a regression.
  (ii)  idle             the new call with nobody lost (the same frames, max_mse = 120) against keyframe_track in the same run, tick by tick on two
                         identical fleets, with a table of 1 and of 60 entries.
  (iii) one in eight     every eighth session is given the kidnapped frame of photo_search_util.kidnapped (lost, and found again on its keyframe): the
                         new call against the alternative of a caller without it: keyframe_track(auto_rekey = 0), then
                         hnet_sessions_keyframe_relocalise_oriented on the lost subset (two uploads, two downloads, two synchronisations)."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def frames_of(seqs, n, t):
    f = t % 8                                                          # frame 8 of the path is frame 0's pose: the path repeats
    return np.stack([seqs[i % 4][0][f] for i in range(n)]), np.stack([seqs[i % 4][2][f if f else 8] for i in range(n)])


def make(e, n, capacity):
    from cuahn_vio_amd.homography_net import HnetSessions
    s = HnetSessions(e, n)
    s.enable_keyframes()
    s.enable_keyframe_map(capacity)
    return s


def track_only(a):
    """(i): one line per K, "K wall device" in ms"""
    import keyframe_util as K
    from cuahn_vio_amd import weights
    from cuahn_vio_amd.homography_net import HnetEngine
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    seqs = [K.sequence("out-and-back", seed) for seed in (1, 2, 5, 11)]
    kw = dict(levels=a.levels, max_iterations=a.iterations)
    for n in a.cameras:
        e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=n)
        s = make(e, n, a.capacity)
        ids = np.arange(n, dtype=np.int32)
        rows = []
        for t in range(a.warmup + a.ticks + 1):
            frames, steps = frames_of(seqs, n, t)
            s.push(ids, frames)
            _, w = timed(lambda: s.keyframe_track(ids, steps, **(dict(max_age=1) if t < a.capacity else dict(auto_rekey=0)), **kw))
            rows.append([w, s.last_keyframe_device_ms()])
        r = np.median(np.array(rows[a.warmup + 1:]), axis=0)
        print(f"TRACK {n} {r[0]:.4f} {r[1]:.4f}", flush=True)
        s.close()
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--capacity", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit for (i)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--track-only", action="store_true", help="(i) alone, on the tree named by --root")
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    sys.path.insert(0, os.path.join(a.root, "tests"))
    if a.track_only:
        return track_only(a)

    # (i) in child processes, this tree and the parent in turn
    trees = [("this tree", HERE)] + ([("parent", os.path.abspath(a.parent))] if a.parent else [])
    got = {name: {n: [] for n in a.cameras} for name, _ in trees}
    common = ["--cameras", *map(str, a.cameras), "--ticks", str(a.ticks), "--warmup", str(a.warmup), "--levels", str(a.levels), "--iterations", str(a.iterations),
              "--capacity", str(a.capacity)]
    for _ in range(a.rounds):
        for name, root in trees:
            env = dict(os.environ)
            env.pop("HNET_LIB_PATH", None)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--track-only", "--root", root, *common], check=True, capture_output=True, text=True,
                                 env=env, cwd=root, timeout=600).stdout
            for line in out.splitlines():
                if line.startswith("TRACK "):
                    _, n, w, d = line.split()
                    got[name][int(n)].append((float(w), float(d)))
    for n in a.cameras:
        for name, _ in trees:
            w, d = zip(*got[name][n])
            print(f"(i) K = {n:3d}, keyframe_track, {name:9s}: wall " + " ".join(f"{x:.4f}" for x in w) + " ms | device " + " ".join(f"{x:.4f}" for x in d) + " ms",
                  flush=True)
        if a.parent:
            for j, what in enumerate(("wall", "device")):
                mine, par = [x[j] for x in got["this tree"][n]], [x[j] for x in got["parent"][n]]
                spread = max(par) - min(par)
                verdict = "REGRESSION" if max(mine) > max(par) + spread else "no regression"
                print(f"    {what}: this tree's largest {max(mine):.4f} ms, the parent's largest {max(par):.4f} ms, the parent's spread {spread:.4f} ms: {verdict}", flush=True)

    import keyframe_util as K
    import photo_search_util as S
    from cuahn_vio_amd import _capi, weights
    from cuahn_vio_amd.homography_net import HnetEngine
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    seqs = [K.sequence("out-and-back", seed) for seed in (1, 2, 5, 11)]
    tables = [_capi.photo_search_yaw_table(0.0, 6.0, 1), _capi.photo_search_yaw_table()]
    kw = dict(levels=a.levels, max_iterations=a.iterations)
    for n in a.cameras:
        e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=n)
        ids = np.arange(n, dtype=np.int32)
        # (ii) nobody lost: fleet 0 tracks, fleets 1 and 2 call the new one with 1 and 60 entries
        fleets = [make(e, n, a.capacity) for _ in range(3)]
        rows, n_lost = [], 0
        for t in range(a.warmup + a.ticks + 1):
            frames, steps = frames_of(seqs, n, t)
            tk = dict(max_age=1) if t < a.capacity else dict(auto_rekey=0)
            row = []
            for i, s in enumerate(fleets):
                s.push(ids, frames)
                if i == 0:
                    _, w = timed(lambda: s.keyframe_track(ids, steps, max_mse=120.0, **tk, **kw))
                else:
                    out, w = timed(lambda: s.keyframe_track_recover(ids, steps, hyps=tables[i - 1], track=dict(max_mse=120.0, **tk, **kw), reloc=kw))
                    n_lost += int(((out["track"]["flags"] & _capi.KF_LOST) != 0).sum())
                row += [w, s.last_keyframe_device_ms()]
            rows.append(row)
        r = np.median(np.array(rows[a.warmup + 1:]), axis=0)
        print(f"(ii) K = {n:3d}, {n_lost} LOST verdicts over the run: keyframe_track wall {r[0]:.4f} ms, device {r[1]:.4f} ms", flush=True)
        for i, tab in enumerate(tables):
            w, d = r[2 + 2 * i], r[3 + 2 * i]
            print(f"    {len(tab):2d} entries: keyframe_track_recover wall {w:.4f} ms ({w - r[0]:+.4f}, {100 * (w - r[0]) / r[0]:+.1f} %), device {d:.4f} ms ({d - r[1]:+.4f}, "
                  f"{100 * (d - r[1]) / r[1]:+.1f} % of the track's; the yardstick is 25 %)", flush=True)
        for s in fleets:
            s.close()
        # (iii) one session in eight lost and recovered: the new call against track(auto_rekey = 0) + relocalise_oriented on the lost subset
        kid = S.kidnapped(5)[0]
        lost = np.arange(0, n, 8, dtype=np.int32)
        a_s, b_s = make(e, n, a.capacity), make(e, n, a.capacity)
        rows, recovered = [], 0
        first, _ = frames_of(seqs, n, 0)
        frames, st = frames_of(seqs, n, 1)
        first[lost], frames[lost], st[lost] = kid[0], kid[1], 0.0
        for t in range(a.warmup + a.ticks + 1):
            row = []
            for s in (a_s, b_s):                                       # every tick starts over: the keyframe at frame 0, then frame 1 in the measured call
                for i in range(n):
                    s.keyframe_reset(i)
                s.push(ids, first)
                s.keyframe_track(ids, None, **kw)
                s.push(ids, frames)
            out, w = timed(lambda: a_s.keyframe_track_recover(ids, st, track=dict(max_mse=120.0, auto_rekey=0, **kw), reloc=kw))
            row += [w, a_s.last_keyframe_device_ms()]
            recovered = int(((out["track"]["flags"] & _capi.KF_RECOVERED) != 0).sum())

            def two_calls():
                tr = b_s.keyframe_track(ids, st, max_mse=120.0, auto_rekey=0, **kw)
                d = b_s.last_keyframe_device_ms()
                sub = ids[(tr["flags"] & _capi.KF_LOST) != 0]
                if len(sub):
                    b_s.keyframe_relocalise_oriented(sub, **kw)
                    d += b_s.last_keyframe_device_ms()
                return d
            d, w = timed(two_calls)
            row += [w, d]
            rows.append(row)
        r = np.median(np.array(rows[a.warmup + 1:]), axis=0)
        print(f"(iii) K = {n:3d}, {len(lost)} lost and {recovered} recovered, 60 entries: keyframe_track_recover wall {r[0]:.4f} ms, device {r[1]:.4f} ms | "
              f"track(auto_rekey = 0) + relocalise_oriented(lost subset) wall {r[2]:.4f} ms, device {r[3]:.4f} ms", flush=True)
        a_s.close()
        b_s.close()
        e.close()


if __name__ == "__main__":
    main()
