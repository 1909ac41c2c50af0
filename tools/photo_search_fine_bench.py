#!/usr/bin/env python3
"""Device time of hnet_sessions_keyframe_relocalise_fine next to the three existing relocalising calls, against a built checkout of the parent commit
(DESIGN 7x), on a GPU:
  python tools/photo_search_fine_bench.py [--cameras 8 64] [--ticks 40] [--warmup 5] [--levels 4] [--iterations 6] [--capacity 3] [--parent DIR] [--rounds 2]
The setting is tools/photo_search_oriented_bench.py's: per K cameras one sessions object with a keyframe map of `capacity` slots, every tick pushes the next
frame of an out-and-back path (4 seeds, cycled) to all K sessions and tracks it (max_age = 1 for the first `capacity` ticks, then auto_rekey = 0); a twin
fleet takes the same frames through hnet_sessions_keyframe_track_recover (nobody is lost: max_mse = 120) under the default table.  Then, per tick and with
max_closure_px = 1e-6 (every candidate is searched, the alignment runs against the pick and the call is REJECTED, so that the next tick's track sees
the state the track left), the device (event) time of
  relocalise                 hnet_sessions_keyframe_relocalise
  oriented 60 x 6            hnet_sessions_keyframe_relocalise_oriented under the default table: what a caller pays today
  oriented 30 x 12           the same under 30 entries of 12 degrees: the coarse stage of the next row alone
  fine 30 x 12, 5, 3         hnet_sessions_keyframe_relocalise_fine (this tree only)
  fine 60 x 6, 5, 3          the same under the default table (this tree only)
Medians over --ticks ticks after --warmup.  Every measurement runs in a process of its own.  The existing calls are measured by the same sequence of calls
in both trees (no fine call in that process); with --parent DIR the two trees run in turn, P T T P per round, and (i) a median of this tree above the
parent's largest by more than the parent's own spread is reported as a regression of an existing call.  (ii) The fine rows come from a further process
of this tree per round, next to oriented 60 x 6 in the same process, and are set against the parent's oriented 60 x 6."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXISTING = ("relocalise", "oriented 60 x 6", "oriented 30 x 12", "track_recover")
FINE = ("fine 30 x 12, 5, 3", "fine 60 x 6, 5, 3")


def child(a):
    """one tree, one process -> a JSON line {K: {row: median device ms}}"""
    sys.path.insert(0, a.child)
    sys.path.insert(0, os.path.join(a.child, "tests"))
    import keyframe_util as K
    from cuahn_vio_amd import _capi, weights
    from cuahn_vio_amd.homography_net import HnetEngine, HnetSessions
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    seqs = [K.sequence("out-and-back", seed) for seed in (1, 2, 5, 11)]
    t60, t30 = _capi.photo_search_yaw_table(), _capi.photo_search_yaw_table(-180.0, 12.0, 30)
    has_fine = a.with_fine
    if has_fine:
        f60, f30 = _capi.photo_search_fine_yaw_table(-180.0, 6.0, 60, 5), _capi.photo_search_fine_yaw_table(-180.0, 12.0, 30, 5)
    result = {}
    for n in a.cameras:
        e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=n)
        fleets = []
        for _ in range(2):
            s = HnetSessions(e, n)
            s.enable_keyframes()
            s.enable_keyframe_map(a.capacity)
            fleets.append(s)
        s, twin = fleets
        ids = np.arange(n, dtype=np.int32)
        kw = dict(levels=a.levels, max_iterations=a.iterations)
        rej = dict(max_closure_px=1e-6, **kw)
        rows = {k: [] for k in (("oriented 60 x 6",) + FINE if has_fine else EXISTING)}
        for t in range(a.warmup + a.ticks + 1):
            f = t % 8                                                  # frame 8 of the path is frame 0's pose: the path repeats
            frames = np.stack([seqs[i % 4][0][f] for i in range(n)])
            steps = np.stack([seqs[i % 4][2][f if f else 8] for i in range(n)])
            track = dict(max_age=1) if t < a.capacity else dict(auto_rekey=0)
            s.push(ids, frames)
            twin.push(ids, frames)
            s.keyframe_track(ids, steps, **track, **kw)
            twin.keyframe_track_recover(ids, steps, hyps=t60, track=dict(max_mse=120.0, **track, **kw), reloc=kw)
            if t <= a.warmup:
                continue
            if not has_fine:
                rows["track_recover"].append(twin.last_keyframe_device_ms())
                s.keyframe_relocalise(ids, **rej)
                rows["relocalise"].append(s.last_keyframe_device_ms())
            for name, tab in (("oriented 60 x 6", t60),) + ((("oriented 30 x 12", t30),) if not has_fine else ()):
                ro = s.keyframe_relocalise_oriented(ids, hyps=tab, **rej)
                rows[name].append(s.last_keyframe_device_ms())
                assert not (ro["rv"]["flags"] & (_capi.RL_ATTACHED | _capi.RL_RETRACKED)).any()
            if has_fine:
                for name, tab, fine in ((FINE[0], t30, f30), (FINE[1], t60, f60)):
                    rf = s.keyframe_relocalise_fine(ids, hyps=tab, fine=fine, fine_opts=dict(n_fine=5, radius=3), **rej)
                    rows[name].append(s.last_keyframe_device_ms())
                    assert not (rf["base"]["rv"]["flags"] & (_capi.RL_ATTACHED | _capi.RL_RETRACKED)).any()
                    assert ((rf["fine"]["flags"] == _capi.PSF_REFINED) == (rf["base"]["target"] != _capi.RL_TARGET_NONE)).all()
        result[str(n)] = {k: float(np.median(v)) for k, v in rows.items()}
        for x in fleets:
            x.close()
        e.close()
    print("RESULT " + json.dumps(result), flush=True)


def run_child(root, a, with_fine=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", root, *(["--with-fine"] if with_fine else []), "--cameras", *map(str, a.cameras),
           "--ticks", str(a.ticks), "--warmup", str(a.warmup), "--levels", str(a.levels), "--iterations", str(a.iterations), "--capacity", str(a.capacity)]
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    if r.returncode != 0:
        sys.exit(f"the measurement of {root} ended with {r.returncode}: {r.stderr[-2000:]}")
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    print(f"  ({'this tree' if root == HERE else 'parent'}{', fine rows' if with_fine else ''}: {time.perf_counter() - t0:.1f} s)", flush=True)
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--capacity", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds one measuring process may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--with-fine", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    order = (["P", "T", "T", "P"] if a.parent else ["T", "T"]) * a.rounds
    runs = {"P": [], "T": [], "F": []}
    for which in order:
        runs[which].append(run_child(a.parent if which == "P" else HERE, a))
    for _ in range(a.rounds):
        runs["F"].append(run_child(HERE, a, with_fine=True))
    print(f"order {' '.join(order)}; levels={a.levels} K_trials={a.iterations} capacity={a.capacity}; device ms, median of {a.ticks} ticks per process", flush=True)
    for n in map(str, a.cameras):
        print(f"K = {n}", flush=True)
        for row in EXISTING:
            t = [r[n][row] for r in runs["T"]]
            line = f"  {row:20s} this tree {min(t):.4f} .. {max(t):.4f} (median {np.median(t):.4f})"
            if runs["P"]:
                p = [r[n][row] for r in runs["P"]]
                over = np.median(t) - max(p)
                verdict = "REGRESSION" if over > max(p) - min(p) else "holds"
                line += f" | parent {min(p):.4f} .. {max(p):.4f} (median {np.median(p):.4f}) | median - parent's largest {over:+.4f}: {verdict}"
            print(line, flush=True)
        base = [r[n]["oriented 60 x 6"] for r in (runs["P"] or runs["T"])]
        same = [r[n]["oriented 60 x 6"] for r in runs["F"]]
        print(f"  (oriented 60 x 6 in the fine rows' processes: {min(same):.4f} .. {max(same):.4f})", flush=True)
        for row in FINE:
            t = [r[n][row] for r in runs["F"]]
            print(f"  {row:20s} this tree {min(t):.4f} .. {max(t):.4f} (median {np.median(t):.4f}) | against {'the parent' if runs['P'] else 'this tree'}'s oriented "
                  f"60 x 6 (median {np.median(base):.4f}): {np.median(t) - np.median(base):+.4f} ms", flush=True)


if __name__ == "__main__":
    main()
