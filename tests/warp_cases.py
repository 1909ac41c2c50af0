"""Inputs and references shared by the warp / prep tests (test_gpu_parity.py, test_gpu_frontend_batch.py): the hostile homographies, the pool of
DLT draws, and AvgPool in the prep kernel's own summation order."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P4 = np.array([0, 0, 0, 223, 319, 223, 319, 0], np.float32)


def nasty_homographies():
    g = np.load(os.path.join(GOLDEN_DIR, "warp_s11.npz"))
    hs = {n: g["H_" + n].astype(np.float32) for n in ("identity", "shift", "oob", "persp")}
    hs["z_zero"] = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]], np.float32)                  # NaN coordinates everywhere
    hs["z_sign_change"] = np.array([[1, 0, 0], [0, 1, 0], [-1 / 160.0, 0, 1]], np.float32)   # Z = 0 on the column u = 160
    hs["zoom_out_3x"] = np.array([[3, 0, -300], [0, 3, -200], [0, 0, 1]], np.float32)       # source box of a tile > staging buffer
    hs["rot90"] = np.array([[0, -1, 270], [1, 0, -50], [0, 0, 1]], np.float32)
    hs["shrink"] = np.array([[0.05, 0, 100], [0, 0.05, 100], [0, 0, 1]], np.float32)        # whole tile inside 4 x 2 source pixels
    hs["far_shift"] = np.array([[1, 0, 5000], [0, 1, 0], [0, 0, 1]], np.float32)
    hs["edge_minus_half"] = np.array([[1, 0, -0.5], [0, 1, -0.5], [0, 0, 1]], np.float32)   # taps at -1 on the first row / column
    return hs


def pool_like_kernel(x, k):
    """AvgPool in the summation order of prep_warp_tiled_kernel: rows of a window sequentially, then a pairwise tree over its columns"""
    h, w = x.shape
    cols = np.zeros((h // k, w), np.float32)
    for i in range(k):
        cols = (cols + x[i::k]).astype(np.float32)
    parts = [cols[:, j::k] for j in range(k)]
    while len(parts) > 1:
        parts = [(parts[2 * j] + parts[2 * j + 1]).astype(np.float32) for j in range(len(parts) // 2)]
    return (parts[0] * np.float32(1.0 / (k * k))).astype(np.float32)


def dlt_draws(seed=2024, per_scale=3, scales=(4.0, 20.0, 80.0)):
    """homographies p4 -> p4 + offsets with corner offsets uniform in +-scale px (float64 solve, rounded to fp32 like the kernels' H), from a seeded
    generator: {name: H [3, 3] float32}"""
    from cuahn_vio_amd import synth
    rng = np.random.default_rng(seed)
    out = {}
    for sc in scales:
        for i in range(per_scale):
            off = rng.uniform(-sc, sc, 8)
            out[f"dlt{int(sc)}_{i}"] = synth.dlt_h(off).astype(np.float32).reshape(3, 3)
    return out


# the homographies test_op_warp_golden_and_oracle holds against the CPU oracle at 2e-4 (the others are hostile: Z = 0 lines, NaN coordinates, where
# the oracle's double arithmetic and the kernel's fp32 legitimately pick other taps)
ORACLE_GATED = ("identity", "shift", "oob", "persp")


def homography_pool():
    """the hostile homographies + the DLT draws; (pool, names the oracle gate applies to)"""
    pool = dict(nasty_homographies())
    draws = dlt_draws()
    pool.update(draws)
    return pool, ORACLE_GATED + tuple(draws)
