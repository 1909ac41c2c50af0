#!/usr/bin/env python3
"""sha256 of the records of the three photometric alignment calls, to compare two trees byte for byte on a GPU:
  python tools/photo_align_out_hash.py [--parent DIR]
One line per call and input: hnet_op_photo_align (K = 0 and 8), hnet_op_photo_align_pyramid (levels 1 - 4, K = 8) and hnet_op_photo_align_robust (levels 1
and 4; model off with huber_k = 0, model on with huber_k = 10; K = 8), `out` and `levels_out` hashed together, on the stock pairs of
tools/photo_align_bench.py at n = 1, 3 and 8 and on the hostile starts of tests/photo_hostile.py.  With --parent DIR (a built checkout of the parent commit)
each tree runs in a fresh child process and every line is compared: the last line says whether all are equal."""
import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hashes(root):
    sys.path.insert(0, os.path.join(root, "tests"))
    sys.path.insert(0, root)
    import photo_hostile as H
    from cuahn_vio_amd import synth, weights
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(weights.pack_state_dict(weights.synthetic_state(0)), variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=16)
    inputs = []
    for n in (1, 3, 8):
        near, far = ([synth.make_pair(1 + i % 16, d) for i in range(n)] for d in (12.0, 32.0))
        prior = np.stack([synth.make_prior(1 + i % 16, near[i][2], 1.0) for i in range(n)])
        inputs.append((f"stock-12px-prior n={n}", np.stack([p[0] for p in near]), np.stack([p[1] for p in near]), prior))
        inputs.append((f"stock-32px-zero n={n}", np.stack([p[0] for p in far]), np.stack([p[1] for p in far]), np.zeros((n, 8), np.float32)))
    starts = H.align_starts()
    s1, s2 = H.pairs()["smooth"]
    inputs.append((f"hostile n={len(starts)}", np.stack([s1] * len(starts)), np.stack([s2] * len(starts)), np.stack([s[1] for s in starts])))
    both = lambda r: np.ascontiguousarray(r[0]).tobytes() + np.ascontiguousarray(r[1]).tobytes()
    for name, i1, i2, start in inputs:
        calls = [(f"align K={k}", lambda k=k: e.op_photo_align(i1, i2, start, max_iterations=k).tobytes()) for k in (0, 8)]
        calls += [(f"pyramid levels={L} K=8", lambda L=L: both(e.op_photo_align_pyramid(i1, i2, start, levels=L, want_levels=True, max_iterations=8)))
                  for L in (1, 2, 3, 4)]
        calls += [(f"robust levels={L} brightness={b} huber_k={k:g} K=8",
                   lambda L=L, b=b, k=k: both(e.op_photo_align_robust(i1, i2, start, levels=L, want_levels=True, max_iterations=8, brightness=b, huber_k=k)))
                  for L in (1, 4) for b, k in ((0, 0.0), (1, 10.0))]
        for what, call in calls:
            print(f"HASH {name} | {what} | {hashlib.sha256(call()).hexdigest()}", flush=True)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--root", default=None, help="hash on the tree in this directory (what --parent starts)")
    a = ap.parse_args()
    if a.root or not a.parent:
        return hashes(a.root or HERE)
    got = {}
    for name, root in (("this tree", HERE), ("parent", os.path.abspath(a.parent))):
        env = dict(os.environ)
        env.pop("HNET_LIB_PATH", None)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root], check=True, capture_output=True, text=True, env=env, cwd=root, timeout=600).stdout
        got[name] = [line[5:] for line in out.splitlines() if line.startswith("HASH ")]
    mine, par = got["this tree"], got["parent"]
    same = 0
    for m, p in zip(mine, par):
        same += m == p
        print(m if m == p else f"DIFFERENT: this tree {m} || parent {p}")
    ok = len(mine) == len(par) and len(mine) > 0 and same == len(mine)
    print(f"{same} of {len(mine)} calls equal between the trees: {'EQUAL' if ok else 'DIFFERENT'}")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
