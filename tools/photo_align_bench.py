#!/usr/bin/env python3
"""Device time of photometric alignment (hnet_op_photo_align) against its yardsticks, on a GPU:
  python tools/photo_align_bench.py [--batches 1 8 64] [--reps 40] [--warmup 5]
per batch n: hnet_last_photo_align_device_ms (HIP events around the launch sequence) at max_iterations 0 and 6, the host wall time of
hnet_op_photo_residual with m = 1 (a call that ends in a synchronise; its kernels' own time comes from a kernel trace) and the device time of one
forward of the same batch (hnet_sessions_last_timing).  Medians over --reps calls after --warmup; stock synthetic pairs started from the sigma = 1 prior.
  python tools/photo_align_bench.py --levels L [--iterations K] [--batches 1 8 64]
the coarse-to-fine call instead (hnet_op_photo_align_pyramid): per batch n the device time of L levels with K trials per level (default 8) on
stock pairs up to 32 px apart, started from zero offsets, with the trials every level made and the worst distance from the truth.
  python tools/photo_align_bench.py --robust [--huber K] [--no-brightness] [--levels L] [--iterations K]
the gain / bias + Huber call (hnet_op_photo_align_robust) on the same pairs, from the same start and with the same trials (levels defaults
to 4), with the gain it found.
  python tools/photo_align_bench.py --parent DIR [--rounds 3] [--batches 1 8 64]
this tree against a built checkout of the parent commit in DIR: the device time of the plain call (K = 0 and 6), the pyramid call (4 levels, K = 8) and the
robust call (1 and 4 levels, K = 8), each tree in fresh child processes in turn, --rounds medians per cell.  A median of this tree above the parent's
largest by more than the parent's own spread reads REGRESSION.
  python tools/photo_align_bench.py --summarize DIR
prints, from the kernel trace a `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/photo_align_bench.py ...` run left in DIR, the mean
duration of every photometric kernel by grid size."""
import argparse
import collections
import csv
import glob
import os
import re
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summarize(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {d}")
    acc = collections.defaultdict(list)
    for r in csv.DictReader(open(files[0])):
        k = re.sub(r"\(.*$", "", re.sub(r"hnet::", "", re.sub(r"^void ", "", r["Kernel_Name"])))
        if "photo" in k:
            dims = lambda name: int(r.get(name + "_X") or 1) * int(r.get(name + "_Y") or 1) * int(r.get(name + "_Z") or 1)      # (work-items)
            grid = int(r["Grid_Size"]) if r.get("Grid_Size") else dims("Grid_Size")
            wg = dims("Workgroup_Size") if r.get("Workgroup_Size_X") else 256
            acc[(k, grid, grid // wg)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    for (k, g, w), v in sorted(acc.items()):
        v = np.array(v)
        print(f"{k:32s} grid {g:7d} ({w:4d} workgroups)  x{len(v):5d}  mean {v.mean():8.2f} us  median {np.median(v):8.2f} us  min {v.min():8.2f} us")


def pyramid(a, blob):
    from cuahn_vio_amd import synth
    from cuahn_vio_amd.homography_net import HnetEngine
    for n in a.batches:
        pairs = [synth.make_pair(1 + i % 16, 32.0) for i in range(n)]
        i1, i2, truth = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), np.stack([p[2] for p in pairs])
        start = np.zeros((n, 8), np.float32)
        e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=n)
        ms = []
        for r in range(a.warmup + a.reps):
            if a.robust:
                rob, lvr = e.op_photo_align_robust(i1, i2, start, levels=a.levels, want_levels=True, max_iterations=a.iterations, huber_k=a.huber,
                                                   brightness=0 if a.no_brightness else 1)
                rec, lv = rob["px"], lvr["px"]
            else:
                rec, lv = e.op_photo_align_pyramid(i1, i2, start, levels=a.levels, want_levels=True, max_iterations=a.iterations)
            ms.append(e.last_photo_align_device_ms())
        ms = np.array(ms[a.warmup:])
        what = f"robust (k={a.huber:g}, brightness {'off' if a.no_brightness else 'on'}, median gain {np.median(rob['gain']):.4f})" if a.robust else "pyramid"
        err = np.abs(rec["offsets_px"].astype(np.float64) - truth).max(axis=1)
        trials = ", ".join(f"L{L} {lv['trials'][:, L].mean():.1f}" for L in range(a.levels - 1, -1, -1))
        print(f"n = {n:3d}: {what} levels={a.levels} K={a.iterations} {np.median(ms):.4f} ms (min {ms.min():.4f}); trials per pair {trials}; "
              f"worst distance from the truth: median {np.median(err):.3f} px, max {err.max():.3f} px", flush=True)
        e.close()


CELLS = ("plain K=0", "plain K=6", "pyramid levels=4 K=8", "robust levels=1 K=8", "robust levels=4 K=8")


def cells_only(a):
    """the cells of --parent on the tree named by --root: one line "CELL n index median_ms" per cell and batch"""
    from cuahn_vio_amd import synth, weights
    from cuahn_vio_amd.homography_net import HnetEngine
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    for n in a.batches:
        near = [synth.make_pair(1 + i % 16, 12.0) for i in range(n)]
        far = [synth.make_pair(1 + i % 16, 32.0) for i in range(n)]
        prior = np.stack([synth.make_prior(1 + i % 16, near[i][2], 1.0) for i in range(n)])
        n1, n2, f1, f2 = (np.stack([p[k] for p in ps]) for ps in (near, far) for k in (0, 1))
        zero = np.zeros((n, 8), np.float32)
        e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=n)
        calls = (lambda: e.op_photo_align(n1, n2, prior, max_iterations=0),
                 lambda: e.op_photo_align(n1, n2, prior, max_iterations=6),
                 lambda: e.op_photo_align_pyramid(f1, f2, zero, levels=4, max_iterations=8),
                 lambda: e.op_photo_align_robust(f1, f2, zero, levels=1, max_iterations=8, huber_k=10.0, brightness=1),
                 lambda: e.op_photo_align_robust(f1, f2, zero, levels=4, max_iterations=8, huber_k=10.0, brightness=1))
        for j, call in enumerate(calls):
            ms = []
            for r in range(a.warmup + a.reps):
                call()
                ms.append(e.last_photo_align_device_ms())
            print(f"CELL {n} {j} {np.median(ms[a.warmup:]):.4f}", flush=True)
        e.close()


def against_parent(a):
    """this tree and the parent in turn, each in fresh child processes, --rounds medians per cell"""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    trees = [("this tree", here), ("parent", os.path.abspath(a.parent))]
    got = {name: collections.defaultdict(list) for name, _ in trees}
    for _ in range(a.rounds):
        for name, root in trees:
            env = dict(os.environ)
            env.pop("HNET_LIB_PATH", None)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--cells-only", "--root", root, "--batches", *map(str, a.batches), "--reps", str(a.reps),
                                  "--warmup", str(a.warmup)], check=True, capture_output=True, text=True, env=env, cwd=root, timeout=600).stdout
            for line in out.splitlines():
                if line.startswith("CELL "):
                    _, n, j, ms = line.split()
                    got[name][(int(n), int(j))].append(float(ms))
    for n in a.batches:
        for j, what in enumerate(CELLS):
            mine, par = got["this tree"][(n, j)], got["parent"][(n, j)]
            spread = max(par) - min(par)
            verdict = "REGRESSION" if max(mine) > max(par) + spread else "no regression"
            print(f"n = {n:3d}, {what:22s}: this tree " + " ".join(f"{x:.4f}" for x in mine) + " ms | parent " + " ".join(f"{x:.4f}" for x in par) +
                  f" ms | largest {max(mine):.4f} against {max(par):.4f}, the parent's spread {spread:.4f}: {verdict}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: the device time of the cells of CELLS on both trees")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cells-only", action="store_true", help="the cells of --parent alone, on the tree named by --root")
    ap.add_argument("--root", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--levels", type=int, default=0)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--robust", action="store_true")
    ap.add_argument("--huber", type=float, default=10.0)
    ap.add_argument("--no-brightness", action="store_true")
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    if a.parent:
        return against_parent(a)
    if a.root:
        sys.path.insert(0, a.root)
    if a.cells_only:
        return cells_only(a)
    from cuahn_vio_amd import synth, weights
    from cuahn_vio_amd.homography_net import HnetEngine, HnetSessions
    blob = weights.pack_state_dict(weights.synthetic_state(0))
    if a.robust and not a.levels:
        a.levels = 4
    if a.levels:
        return pyramid(a, blob)
    for n in a.batches:
        pairs = [synth.make_pair(1 + i % 16, 12.0) for i in range(n)]
        i1, i2 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        start = np.stack([synth.make_prior(1 + i % 16, pairs[i][2], 1.0) for i in range(n)])
        e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=n)
        s = HnetSessions(e, n)
        ids = np.arange(n, dtype=np.int32)
        s.push(ids, i1, t=[1.0] * n)
        s.push(ids, i2, t=[2.0] * n)
        row = {}
        for K in (0, 6):
            ms = []
            for r in range(a.warmup + a.reps):
                rec = e.op_photo_align(i1, i2, start, max_iterations=K)
                ms.append(e.last_photo_align_device_ms())
            ms = np.array(ms[a.warmup:])
            row[K] = (float(np.median(ms)), float(ms.min()), float(rec["trials"].mean()), int((rec["flags"] & 1).sum()))
        wall = []
        for r in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            e.op_photo_residual(i1, i2, start[:, None, :])
            wall.append((time.perf_counter() - t0) * 1e3)
        wall = np.array(wall[a.warmup:])
        fwd = []
        for r in range(a.warmup + a.reps // 2):
            s.infer(ids, start.astype(np.float64))
            fwd.append(s.last_timing()["device_ms"])
        fwd = np.array(fwd[a.warmup:])
        print(f"n = {n:3d}: align K=0 {row[0][0]:.4f} ms (min {row[0][1]:.4f}); align K=6 {row[6][0]:.4f} ms (min {row[6][1]:.4f}; {row[6][2]:.1f} trials per pair, "
              f"{row[6][3]} converged); residual m=1 call (host wall, with its copies) {np.median(wall):.4f} ms; one forward {np.median(fwd):.4f} ms (device)", flush=True)
        s.close()
        e.close()


if __name__ == "__main__":
    main()
