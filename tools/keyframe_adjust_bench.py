#!/usr/bin/env python3
"""Wall and device time of hnet_sessions_keyframe_adjust, on a GPU:
  python tools/keyframe_adjust_bench.py [--cameras 8 64] [--calls 40] [--warmup 5] [--rounds 3] [--parent DIR] [--bench]
The setting: per K cameras one sessions object with a map of capacity 8; every session tracks 8 frames of an out-and-back path (4 seeds, cycled) with
max_age = 1, so that all 8 entries of every map are valid and all 28 pairs of a session overlap.  Then --calls adjustments of all K sessions with the
default options (apply = 0: every call sees the same map).
  (i)   adjust      medians over the calls of the wall time and of hnet_sessions_last_keyframe_device_ms, one process per round (--rounds of them); the
                    jobs and rounds of a call; and the solve alone: the median wall time of hnet_op_keyframe_adjust_solve on one session's entries,
                    edges and information matrices (one upload, the solve kernel, one download: an upper bound of the kernel's own time, which does
                    not grow with K below one workgroup per CU).
  (ii)  untouched   with --parent DIR (a built checkout of the parent commit): the plain filter step of tools/filters_keyframe_bench.py --step-only on
                    this tree and on the parent in turn, --rounds times.  A median of this tree above the parent's largest by more than the parent's
                    own spread is a regression (7v's rule).
  (iii) --bench     bench.py --gpus 1 --steps 20 --warmup 5 on this tree and the parent in the order T P T P: the result lines' value."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def adjust_only(a):
    """(i) in this process: one line per K, "ADJUST K wall device jobs rounds solve_wall trials" in ms"""
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import keyframe_util as K
    from cuahn_vio_amd import _capi, weights
    from cuahn_vio_amd.homography_net import HnetEngine, HnetSessions
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    seqs = [K.sequence("out-and-back", seed) for seed in (1, 2, 5, 11)]
    for n in a.cameras:
        e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=n)
        s = HnetSessions(e, n)
        s.enable_keyframes()
        s.enable_keyframe_map(8)
        s.enable_keyframe_adjust()
        ids = np.arange(n, dtype=np.int32)
        for f in range(8):
            s.push(ids, np.stack([seqs[i % 4][0][f] for i in range(n)]))
            s.keyframe_track(ids, np.stack([seqs[i % 4][2][f] for i in range(n)]), max_age=1, levels=3, max_iterations=6)
        assert all(int(s.keyframe_map_info(i)[0]["valid"].sum()) == 8 for i in range(min(n, 4)))
        rows, rec = [], None
        for _ in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            rec = s.keyframe_adjust(ids)
            rows.append([(time.perf_counter() - t0) * 1e3, s.last_keyframe_device_ms()])
        r = np.median(np.array(rows[a.warmup:]), axis=0)
        jobs = int(rec["n_jobs"].sum())
        assert (rec["flags"] & (_capi.ADJ_ADJUSTED | _capi.ADJ_NO_GAIN)).all() and (rec["n_jobs"] == 28).all()
        # the solve alone, on session 0's table as the call left it
        rec0, er = s.keyframe_adjust([0], want_edge_records=True)
        ent = s.keyframe_map_info(0)[0]
        edges, infos = rec0[0]["edge"][:28], er[0]["px"]["info"][:28]
        solo = []
        for _ in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            one = e.op_keyframe_adjust_solve(ent, edges, infos)
            solo.append((time.perf_counter() - t0) * 1e3)
        assert one[0]["delta_px"].tobytes() == rec0[0]["delta_px"].tobytes()
        print(f"ADJUST {n} {r[0]:.4f} {r[1]:.4f} {jobs} {-(-jobs // n)} {np.median(solo[a.warmup:]):.4f} {int(rec0[0]['trials'])}", flush=True)
        s.close()
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=40, help="(ii): ticks of the plain filter step per process")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit for (ii) and (iii)")
    ap.add_argument("--bench", action="store_true", help="(iii) as well")
    ap.add_argument("--adjust-only", action="store_true", help="(i) alone, in this process")
    a = ap.parse_args()
    if a.adjust_only:
        return adjust_only(a)
    env = dict(os.environ)
    env.pop("HNET_LIB_PATH", None)

    got = {}
    common = ["--cameras", *map(str, a.cameras), "--calls", str(a.calls), "--warmup", str(a.warmup)]
    for _ in range(a.rounds):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--adjust-only", *common], check=True, capture_output=True, text=True, env=env, cwd=HERE,
                             timeout=600).stdout
        for line in out.splitlines():
            if line.startswith("ADJUST "):
                _, n, w, d, jobs, rounds, solo, trials = line.split()
                got.setdefault(int(n), []).append((float(w), float(d), int(jobs), int(rounds), float(solo), int(trials)))
    for n, rows in got.items():
        w, d, jobs, rounds, solo, trials = zip(*rows)
        print(f"(i) K = {n:3d}, capacity 8, all valid, defaults: wall " + " ".join(f"{x:.4f}" for x in w) + " ms | device " + " ".join(f"{x:.4f}" for x in d) +
              f" ms | {jobs[0]} jobs in {rounds[0]} rounds of {n}, {float(np.median(d)) / rounds[0]:.4f} ms of device time per round | the solve alone "
              f"(operator call, one session, {trials[0]} trials): wall " + " ".join(f"{x:.4f}" for x in solo) + " ms", flush=True)

    trees = [("this tree", HERE)] + ([("parent", os.path.abspath(a.parent))] if a.parent else [])
    if a.parent:
        steps = {name: {n: [] for n in a.cameras} for name, _ in trees}
        for _ in range(a.rounds):
            for name, root in trees:
                out = subprocess.run([sys.executable, os.path.join(root, "tools", "filters_keyframe_bench.py"), "--step-only", "--root", root, "--cameras",
                                      *map(str, a.cameras), "--ticks", str(a.ticks), "--warmup", str(a.warmup)], check=True, capture_output=True, text=True, env=env,
                                     cwd=root, timeout=600).stdout
                for line in out.splitlines():
                    if line.startswith("STEP "):
                        _, n, w, d = line.split()
                        steps[name][int(n)].append((float(w), float(d)))
        for n in a.cameras:
            for name, _ in trees:
                w, d = zip(*steps[name][n])
                print(f"(ii) K = {n:3d}, plain filter step, {name:9s}: wall " + " ".join(f"{x:.4f}" for x in w) + " ms | device " + " ".join(f"{x:.4f}" for x in d) + " ms",
                      flush=True)
            for j, what in enumerate(("wall", "device")):
                mine, par = [x[j] for x in steps["this tree"][n]], [x[j] for x in steps["parent"][n]]
                spread = max(par) - min(par)
                verdict = "REGRESSION" if max(mine) > max(par) + spread else "no regression"
                print(f"    {what}: this tree's largest {max(mine):.4f} ms, the parent's largest {max(par):.4f} ms, the parent's spread {spread:.4f} ms: {verdict}", flush=True)

    if a.bench:
        order = [trees[0], trees[-1]] * 2 if a.parent else [trees[0]] * 2
        for name, root in order:
            out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True, text=True, env=env,
                                 cwd=root, timeout=900)
            line = next((x for x in reversed(out.stdout.splitlines()) if x.startswith("{")), None)
            if out.returncode != 0 or line is None:
                print(f"(iii) bench.py, {name}: exit status {out.returncode}: {out.stderr[-400:]}", flush=True)
                continue
            res = json.loads(line)
            print(f"(iii) bench.py --gpus 1 --steps 20 --warmup 5, {name:9s}: value {res.get('value')} {res.get('unit', '')}, latency p50 {res.get('latency_p50_ms')} ms", flush=True)


if __name__ == "__main__":
    main()
