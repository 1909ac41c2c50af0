#!/usr/bin/env python3
"""Wall and device time of hnet_filters_step with recovery inside the in-step keyframe track, on a GPU:
  python tools/filters_keyframe_recover_bench.py [--cameras 8 64] [--ticks 40] [--warmup 5] [--iters 1] [--parent DIR] [--rounds 3] [--bench] [--untouched-only]
The setting is tools/filters_keyframe_bench.py's: per K cameras one sessions object with keyframes enabled and one filters object; every tick pushes the
next frame of an out-and-back path (4 seeds, cycled) to all K sessions, sets each state just before the frame and steps without an IMU interval.  The
track options are the kidnapped row's (levels 3, auto_rekey 1, max_mse 120).  Medians over --ticks ticks after --warmup, wall and device time.
  (i)   never touched    two configurations, each in a process of its own: the step of a filters object that never heard of keyframes, and a 7v
                         measuring tick on which recovery was never set.  With --parent DIR (a built checkout of the parent commit) the same
                         measurements run on that tree, the two in turn --rounds times: a median of this tree above the parent's largest by more than
                         the parent's own spread is a regression.
  (ii)  idle             recovery on and nobody lost, against the measuring tick on an identical fleet in the same run.  Recorded.
  (iii) one in eight     every eighth session alternates between the kidnapped row's keyframe view and its kidnapped view, so that it is lost and
                         recovered on every tick, against the same tick on a fleet where those sessions have recovery off.  Recorded.
  (iv)  --bench          bench.py --gpus 1 --steps 20 --warmup 5 on this tree and the parent in the order T P T P: the result lines' value."""
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


def measure_opts(_capi):
    return _capi.keyframe_measure_opts(cov_scale=1.0, levels=3, max_iterations=6, auto_rekey=1, track_max_mse=120.0)


def step_only(a):
    """(i): one line per K, "STEP K wall device" in ms; --measuring: every session measures (7v), recovery never set"""
    import keyframe_util as K
    from cuahn_vio_amd import _capi, weights
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    seqs = [K.sequence("out-and-back", seed) for seed in (1, 2, 5, 11)]
    for n in a.cameras:
        e, s, f = fleet(blob, n, a.iters, a.measuring)
        ids = np.arange(n, dtype=np.int32)
        if a.measuring:
            for i in range(n):
                f.set_keyframe_measure(i, measure_opts(_capi))
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
    ap.add_argument("--measuring", action="store_true", help="with --step-only: the 7v measuring tick")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit for (i) and (iv)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench", action="store_true", help="(iv) as well")
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
    common = ["--cameras", *map(str, a.cameras), "--ticks", str(a.ticks), "--warmup", str(a.warmup), "--iters", str(a.iters)]
    for label, extra in (("step, feature never touched", []), ("7v measuring tick, recovery never set", ["--measuring"])):
        got = {name: {n: [] for n in a.cameras} for name, _ in trees}
        for _ in range(a.rounds):
            for name, root in trees:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-only", "--root", root, *common, *extra], check=True, capture_output=True,
                                     text=True, env=env, cwd=root, timeout=600).stdout
                for line in out.splitlines():
                    if line.startswith("STEP "):
                        _, n, w, d = line.split()
                        got[name][int(n)].append((float(w), float(d)))
        for n in a.cameras:
            for name, _ in trees:
                w, d = zip(*got[name][n])
                print(f"(i) K = {n:3d}, {label}, {name:9s}: wall " + " ".join(f"{x:.4f}" for x in w) + " ms | device " + " ".join(f"{x:.4f}" for x in d) + " ms", flush=True)
            if a.parent:
                for j, what in enumerate(("wall", "device")):
                    mine, par = [x[j] for x in got["this tree"][n]], [x[j] for x in got["parent"][n]]
                    spread = max(par) - min(par)
                    verdict = "REGRESSION" if max(mine) > max(par) + spread else "no regression"
                    print(f"    {what}: this tree's largest {max(mine):.4f} ms, the parent's largest {max(par):.4f} ms, the parent's spread {spread:.4f} ms: {verdict}",
                          flush=True)

    if a.untouched_only:
        return
    import keyframe_recover_util as KR
    import keyframe_util as K
    from cuahn_vio_amd import _capi, weights
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    seqs = [K.sequence("out-and-back", seed) for seed in (1, 2, 5, 11)]
    kd = KR.row("kidnapped", 5)["frames"]
    ro = KR.reloc_opts("kidnapped")
    for case in ("idle", "one in eight"):
        for n in a.cameras:
            ids = np.arange(n, dtype=np.int32)
            base, rec = fleet(blob, n, a.iters, True), fleet(blob, n, a.iters, True)
            hit = [i for i in range(n) if i % 8 == 0] if case == "one in eight" else []
            for i in range(n):
                for which, (_, _, f) in enumerate((base, rec)):
                    f.set_keyframe_measure(i, measure_opts(_capi))
                    if which == 1 or (case == "one in eight" and i not in hit):
                        f.set_keyframe_recover(i, ro)
            rows, recovered, lost = [], 0, 0
            for t in range(a.warmup + a.ticks + 2):
                frames, steps = frames_of(seqs, n, t)
                frames, steps = frames.copy(), steps.copy()
                for i in hit:
                    frames[i], steps[i] = kd[t & 1], 0.0
                if t == 0:
                    for _, s, _f in (base, rec):
                        s.push(ids, frames, t=[0.9] * n)
                    continue
                row = []
                for which, (e, s, f) in enumerate((base, rec)):
                    _, w = tick(_capi, s, f, ids, frames, steps, 1.0 + 0.1 * t)
                    row += [w, f.last_timing()["device_ms"]]
                    tf = f.last_keyframe_measure(n)["track"]["flags"]
                    if which == 1:
                        recovered += int(((tf & _capi.KF_RECOVERED) != 0).sum())
                    else:
                        lost += int(((tf & _capi.KF_LOST) != 0).sum())
                rows.append(row)
            r = np.median(np.array(rows[a.warmup:]), axis=0)
            tag = "(ii)" if case == "idle" else "(iii)"
            what = "measuring tick" if case == "idle" else "the tick with those sessions unrecovered"
            print(f"{tag} K = {n:3d}, {case}: {what} wall {r[0]:.4f} ms, device {r[1]:.4f} ms ({lost} lost frames) | recovery on: wall {r[2]:.4f} ms ({r[2] - r[0]:+.4f}), "
                  f"device {r[3]:.4f} ms ({r[3] - r[1]:+.4f}; {(r[3] - r[1]) / r[1]:.2f} of the tick's device median), {recovered} frames recovered", flush=True)
            for fl in (base, rec):
                for x in reversed(fl):
                    x.close()

    if a.bench:
        order = [trees[0], trees[-1]] * 2 if a.parent else [trees[0]] * 2
        for name, root in order:
            out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True, text=True, env=env,
                                 cwd=root, timeout=900)
            line = next((x for x in reversed(out.stdout.splitlines()) if x.startswith("{")), None)
            if out.returncode != 0 or line is None:
                print(f"(iv) bench.py, {name}: exit status {out.returncode}: {out.stderr[-400:]}", flush=True)
                continue
            res = json.loads(line)
            print(f"(iv) bench.py --gpus 1 --steps 20 --warmup 5, {name:9s}: value {res.get('value')} {res.get('unit', '')}", flush=True)


if __name__ == "__main__":
    main()
