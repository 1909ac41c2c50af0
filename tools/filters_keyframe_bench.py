#!/usr/bin/env python3
"""Wall and device time of hnet_filters_step with the keyframe track as an in-step measurement, on a GPU:
  python tools/filters_keyframe_bench.py [--cameras 8 64] [--ticks 40] [--warmup 5] [--iters 1] [--levels 3] [--iterations 6] [--parent DIR] [--rounds 3] [--bench] [--untouched-only]
The setting: per K cameras one sessions object with keyframes enabled and one filters object; every tick pushes the next frame of an out-and-back path
(4 seeds, cycled) to all K sessions, sets each state just before the frame (offsets at the noisy step) and steps without an IMU interval.  Medians over
--ticks ticks after --warmup, wall and device (hnet_filters_last_timing) time.
  (i)   untouched        the step of a filters object that never heard of the feature, in a process of its own.  With --parent DIR (a built checkout of the
                         parent commit) the same measurement runs on that tree's package and library, the two in turn --rounds times: a median of this
                         tree above the parent's largest by more than the parent's own spread is a regression.  The parent is the yardstick.
  (ii)  measuring        the same tick with every session measuring (when = ALWAYS) against the tick without, on two identical fleets in one run; and
                         against the operator's alternative: the step, then hnet_sessions_keyframe_track with the step's mean, nothing fed back (two
                         uploads, two downloads, two synchronisations).  Recorded, not gated.
  (iii) --bench          bench.py --gpus 1 --steps 20 --warmup 5 on this tree and the parent in the order T P T P: the result lines' value."""
import argparse
import json
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


def fleet(blob, n, iters, keyframes):
    from cuahn_vio_amd.homography_net import HnetEngine, HnetFilters, HnetSessions
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=n)
    s = HnetSessions(e, n)
    f = HnetFilters(s, iters)
    if keyframes:
        s.enable_keyframes()
    return e, s, f


def state_for(_capi, step_px, t):
    st = np.zeros(1, _capi.FILTER_STATE_DTYPE)
    st["t"] = t
    st["q"][0][0] = 1.0
    st["offset"][0][:, :2] = np.asarray(step_px, np.float64).reshape(4, 2) / 159.5
    st["cov"][0] = np.eye(27) * 1e-4
    return st


def tick(_capi, s, f, ids, frames, steps, t):
    n = len(ids)
    s.push(ids, frames, t=[t] * n)
    for i in range(n):
        f.set_state(i, state_for(_capi, steps[i], t - 0.05))
    empty = np.zeros(0, _capi.IMU_DTYPE)
    return timed(lambda: f.step(ids, [t] * n, [empty] * n))


def step_only(a):
    """(i): one line per K, "STEP K wall device" in ms"""
    import keyframe_util as K
    from cuahn_vio_amd import _capi, weights
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    seqs = [K.sequence("out-and-back", seed) for seed in (1, 2, 5, 11)]
    for n in a.cameras:
        e, s, f = fleet(blob, n, a.iters, False)
        ids = np.arange(n, dtype=np.int32)
        rows = []
        for t in range(a.warmup + a.ticks + 2):
            frames, steps = frames_of(seqs, n, t)
            if t == 0:
                s.push(ids, frames, t=[0.9] * n)                       # (a step needs a pair)
                continue
            _, w = tick(_capi, s, f, ids, frames, steps, 1.0 + 0.1 * t)
            rows.append([w, f.last_timing()["device_ms"]])
        r = np.median(np.array(rows[a.warmup:]), axis=0)
        print(f"STEP {n} {r[0]:.4f} {r[1]:.4f}", flush=True)
        for x in (f, s, e):
            x.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit for (i) and (iii)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench", action="store_true", help="(iii) as well")
    ap.add_argument("--untouched-only", action="store_true", help="(i) alone: this tree and the parent in turn")
    ap.add_argument("--step-only", action="store_true", help="(i) alone, on the tree named by --root")
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    sys.path.insert(0, os.path.join(a.root, "tests"))
    if a.step_only:
        return step_only(a)

    trees = [("this tree", HERE)] + ([("parent", os.path.abspath(a.parent))] if a.parent else [])
    env = dict(os.environ)
    env.pop("HNET_LIB_PATH", None)
    got = {name: {n: [] for n in a.cameras} for name, _ in trees}
    common = ["--cameras", *map(str, a.cameras), "--ticks", str(a.ticks), "--warmup", str(a.warmup), "--iters", str(a.iters)]
    for _ in range(a.rounds):
        for name, root in trees:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-only", "--root", root, *common], check=True, capture_output=True, text=True,
                                 env=env, cwd=root, timeout=600).stdout
            for line in out.splitlines():
                if line.startswith("STEP "):
                    _, n, w, d = line.split()
                    got[name][int(n)].append((float(w), float(d)))
    for n in a.cameras:
        for name, _ in trees:
            w, d = zip(*got[name][n])
            print(f"(i) K = {n:3d}, step, feature untouched, {name:9s}: wall " + " ".join(f"{x:.4f}" for x in w) + " ms | device " + " ".join(f"{x:.4f}" for x in d) + " ms",
                  flush=True)
        if a.parent:
            for j, what in enumerate(("wall", "device")):
                mine, par = [x[j] for x in got["this tree"][n]], [x[j] for x in got["parent"][n]]
                spread = max(par) - min(par)
                verdict = "REGRESSION" if max(mine) > max(par) + spread else "no regression"
                print(f"    {what}: this tree's largest {max(mine):.4f} ms, the parent's largest {max(par):.4f} ms, the parent's spread {spread:.4f} ms: {verdict}", flush=True)

    if a.untouched_only:
        return
    import keyframe_util as K
    from cuahn_vio_amd import _capi, weights
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    seqs = [K.sequence("out-and-back", seed) for seed in (1, 2, 5, 11)]
    kw = dict(levels=a.levels, max_iterations=a.iterations)
    for n in a.cameras:
        ids = np.arange(n, dtype=np.int32)
        plain, meas, alt = fleet(blob, n, a.iters, True), fleet(blob, n, a.iters, True), fleet(blob, n, a.iters, True)
        for i in range(n):
            meas[2].set_keyframe_measure(i, _capi.keyframe_measure_opts(cov_scale=1.0, auto_rekey=0, **kw))
        rows, applied = [], 0
        for t in range(a.warmup + a.ticks + 2):
            frames, steps = frames_of(seqs, n, t)
            if t == 0:
                for _, s, _f in (plain, meas, alt):
                    s.push(ids, frames, t=[0.9] * n)
                continue
            tt = 1.0 + 0.1 * t
            row = []
            for which, (e, s, f) in enumerate((plain, meas)):
                _, w = tick(_capi, s, f, ids, frames, steps, tt)
                row += [w, f.last_timing()["device_ms"]]
                if which == 1:
                    applied += int(((f.last_keyframe_measure(n)["flags"] & _capi.KFM_APPLIED) != 0).sum())
            e, s, f = alt
            (out, w0) = tick(_capi, s, f, ids, frames, steps, tt)
            d0 = f.last_timing()["device_ms"]
            _, w1 = timed(lambda: s.keyframe_track(ids, out[1][-1][:, :8], auto_rekey=0, **kw))
            row += [w0 + w1, d0 + s.last_keyframe_device_ms()]
            rows.append(row)
        r = np.median(np.array(rows[a.warmup:]), axis=0)
        print(f"(ii) K = {n:3d}, {applied} measurements applied over the run: step wall {r[0]:.4f} ms, device {r[1]:.4f} ms | measuring step wall {r[2]:.4f} ms "
              f"({r[2] - r[0]:+.4f}), device {r[3]:.4f} ms ({r[3] - r[1]:+.4f}) | step + keyframe_track, nothing fed back: wall {r[4]:.4f} ms, device {r[5]:.4f} ms",
              flush=True)
        for fl in (plain, meas, alt):
            for x in reversed(fl):
                x.close()

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
