#!/usr/bin/env python3
"""Wall and device time of hnet_op_photo_align_masked beside hnet_op_photo_align_robust, on a GPU:
  python tools/photo_masked_bench.py [--pairs 1 8] [--calls 40] [--warmup 5] [--rounds 3] [--parent DIR] [--bench] [--trace-only MASK]
The setting: n pairs of the block-4levels accuracy row (exposure step and a foreign block, seeds cycled), 3 levels, 6 trials, robust defaults, from their row's
starts.  The robust call is the yardstick: the same launch sequence without the mask pyramid and with the unmasked accumulate kernels.
  (i)   masked      per n and per mask (full; rows 0 - 95 zero: three of the seven row slices return early at every level; a checkerboard: levels 1 - 3 are
                    empty), medians over the calls of the wall time and of hnet_last_photo_align_device_ms, for the masked call and, in the same process
                    and alternating with it, the robust call on the same pairs; one process per round (--rounds of them).
  (ii)  untouched   with --parent DIR (a built checkout of the parent commit): the plain filter step of tools/filters_keyframe_bench.py --step-only on
                    this tree and on the parent in turn, --rounds times, and hnet_op_photo_align_robust of tools/photo_masked_bench.py's pairs on both (its
                    translation unit gained the third form of the level driver).  A median of this tree above the parent's largest by more than the
                    parent's own spread is a regression (7v's rule).
  (iii) --bench     bench.py --gpus 1 --steps 20 --warmup 5 on this tree and the parent in the order T P T P: the result lines' value.
  --trace-only MASK one process that makes 20 masked and 20 robust calls of n = the largest of --pairs on MASK and nothing else: the workload of a
                    `rocprofv3 --kernel-trace --stats -d DIR -- python tools/photo_masked_bench.py --trace-only rows-0-95-zero` run of its own."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS, TRIALS = 3, 6
MASKS = ("full", "rows-0-95-zero", "checkerboard")


def _setting(root, n):
    """-> (engine, img1, img2, start) of n pairs on the tree `root`"""
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import photo_robust_util as R
    from cuahn_vio_amd import weights
    from cuahn_vio_amd.homography_net import HnetEngine
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    i1, i2, _, start = R.row_pairs("block-4levels")
    pick = [i % 4 for i in range(n)]
    return HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=n), i1[pick], i2[pick], start[pick]


def masked_only(a):
    """(i) in this process: one line per n and mask, "MASKED n mask wall device robust_wall robust_device" in ms"""
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import photo_masked_util as M
    for n in a.pairs:
        e, i1, i2, start = _setting(HERE, n)
        for name in MASKS:
            mask = np.stack([M.masks()[name]] * n)
            rows = []
            for _ in range(a.warmup + a.calls):
                t0 = time.perf_counter()
                e.op_photo_align_masked(i1, mask, i2, start, levels=LEVELS, max_iterations=TRIALS)
                t1 = time.perf_counter()
                dm = e.last_photo_align_device_ms()
                e.op_photo_align_robust(i1, i2, start, levels=LEVELS, max_iterations=TRIALS)
                rows.append([(t1 - t0) * 1e3, dm, (time.perf_counter() - t1) * 1e3, e.last_photo_align_device_ms()])
            r = np.median(np.array(rows[a.warmup:]), axis=0)
            print(f"MASKED {n} {name} {r[0]:.4f} {r[1]:.4f} {r[2]:.4f} {r[3]:.4f}", flush=True)
        e.close()


def robust_only(a):
    """(ii)'s alignment part in this process, on the tree --root: "ROBUST n wall device" in ms"""
    for n in a.pairs:
        e, i1, i2, start = _setting(a.root, n)
        rows = []
        for _ in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            e.op_photo_align_robust(i1, i2, start, levels=LEVELS, max_iterations=TRIALS)
            rows.append([(time.perf_counter() - t0) * 1e3, e.last_photo_align_device_ms()])
        r = np.median(np.array(rows[a.warmup:]), axis=0)
        print(f"ROBUST {n} {r[0]:.4f} {r[1]:.4f}", flush=True)
        e.close()


def trace_only(name, n):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import photo_masked_util as M
    e, i1, i2, start = _setting(HERE, n)
    mask = np.stack([M.masks()[name]] * n)
    for _ in range(20):
        e.op_photo_align_masked(i1, mask, i2, start, levels=LEVELS, max_iterations=TRIALS)
        e.op_photo_align_robust(i1, i2, start, levels=LEVELS, max_iterations=TRIALS)
    e.close()


def _tick(what):
    print(f"[{time.strftime('%H:%M:%S')}] {what}", file=sys.stderr, flush=True)      # (progress, so that a long quiet stretch is not taken for a hang)


def _verdict(label, mine, par):
    spread = max(par) - min(par)
    verdict = "REGRESSION" if max(mine) > max(par) + spread else "no regression"
    print(f"    {label}: this tree's largest {max(mine):.4f} ms, the parent's largest {max(par):.4f} ms, the parent's spread {spread:.4f} ms: {verdict}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--cameras", type=int, nargs="+", default=[8, 64], help="(ii): cameras of the plain filter step")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=40, help="(ii): ticks of the plain filter step per process")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit for (ii) and (iii)")
    ap.add_argument("--bench", action="store_true", help="(iii) as well")
    ap.add_argument("--masked-only", action="store_true", help="(i) alone, in this process")
    ap.add_argument("--robust-only", action="store_true", help="the robust call alone, in this process, on --root")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--trace-only", default=None, choices=MASKS)
    a = ap.parse_args()
    if a.masked_only:
        return masked_only(a)
    if a.robust_only:
        return robust_only(a)
    if a.trace_only:
        return trace_only(a.trace_only, max(a.pairs))
    env = dict(os.environ)
    env.pop("HNET_LIB_PATH", None)
    me = os.path.abspath(__file__)
    common = ["--pairs", *map(str, a.pairs), "--calls", str(a.calls), "--warmup", str(a.warmup)]

    got = {}
    for r in range(a.rounds):
        _tick(f"(i) round {r}")
        out = subprocess.run([sys.executable, me, "--masked-only", *common], check=True, capture_output=True, text=True, env=env, cwd=HERE, timeout=600).stdout
        for line in out.splitlines():
            if line.startswith("MASKED "):
                _, n, name, w, d, rw, rd = line.split()
                got.setdefault((int(n), name), []).append((float(w), float(d), float(rw), float(rd)))
    for (n, name), rows in got.items():
        w, d, rw, rd = zip(*rows)
        print(f"(i) n = {n}, mask {name:15s}: masked wall " + " ".join(f"{x:.4f}" for x in w) + " ms | device " + " ".join(f"{x:.4f}" for x in d) +
              " ms || robust wall " + " ".join(f"{x:.4f}" for x in rw) + " ms | device " + " ".join(f"{x:.4f}" for x in rd) + " ms", flush=True)

    trees = [("this tree", HERE)] + ([("parent", os.path.abspath(a.parent))] if a.parent else [])
    if a.parent:
        steps = {name: {n: [] for n in a.cameras} for name, _ in trees}
        rob = {name: {n: [] for n in a.pairs} for name, _ in trees}
        for _ in range(a.rounds):
            for name, root in trees:
                _tick(f"(ii) {name}")
                out = subprocess.run([sys.executable, os.path.join(root, "tools", "filters_keyframe_bench.py"), "--step-only", "--root", root, "--cameras",
                                      *map(str, a.cameras), "--ticks", str(a.ticks), "--warmup", str(a.warmup)], check=True, capture_output=True, text=True, env=env,
                                     cwd=root, timeout=600).stdout
                for line in out.splitlines():
                    if line.startswith("STEP "):
                        _, n, w, d = line.split()
                        steps[name][int(n)].append((float(w), float(d)))
                out = subprocess.run([sys.executable, me, "--robust-only", "--root", root, *common], check=True, capture_output=True, text=True, env=env, cwd=root,
                                     timeout=600).stdout
                for line in out.splitlines():
                    if line.startswith("ROBUST "):
                        _, n, w, d = line.split()
                        rob[name][int(n)].append((float(w), float(d)))
        for what, table, keys in (("plain filter step, K", steps, a.cameras), ("hnet_op_photo_align_robust, n", rob, a.pairs)):
            for n in keys:
                for name, _ in trees:
                    w, d = zip(*table[name][n])
                    print(f"(ii) {what} = {n:3d}, {name:9s}: wall " + " ".join(f"{x:.4f}" for x in w) + " ms | device " + " ".join(f"{x:.4f}" for x in d) + " ms", flush=True)
                for j, label in enumerate(("wall", "device")):
                    _verdict(label, [x[j] for x in table["this tree"][n]], [x[j] for x in table["parent"][n]])

    if a.bench:
        order = [trees[0], trees[-1]] * 2 if a.parent else [trees[0]] * 2
        for name, root in order:
            _tick(f"(iii) {name}")
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
