"""What the CPU and the GPU tests of photometric alignment with a gain / bias model and Huber weights share (include/hnet.h hnet_op_photo_align_robust;
DESIGN 7n): the spoiled pairs, the accuracy rows and their gates, the hostile starts, the host reference tests/cpp/photo_robust_ref.cpp behind ctypes, and the
record layouts."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import photo_align_pyr_util as P
import photo_align_util as U
from cuahn_vio_amd import _capi

ROOT = U.ROOT
REC = _capi.PHOTO_ROBUST_DTYPE
SUMS = np.dtype([("tt", "<f8", 66), ("tr", "<f8", 11), ("rho", "<f8"), ("n_valid", "<i4"), ("n_outliers", "<i4")])
assert REC.itemsize == 1560 and SUMS.itemsize == 632
GAIN, BIAS, BLOCK, HUBER_K = 0.7, 25.0, (60, 100, 40, 60), 10.0          # the exposure step and the foreign block (row, column, rows, columns) of the accuracy rows
RATIO = 3.0                                                             # hnet_op_photo_align_pyramid must end at least this many times further from the truth

# The accuracy rows: name -> (levels, max_iterations, block, huber_k, gate in px).  A gate is TWICE the worst distance from the truth (worst component, px)
# of the host reference over seeds 1, 2, 5, 11, as tests/test_photo_robust_cpu.py::test_accuracy_rows prints it (DESIGN 7n holds the measured values)
ROWS = {
    "gain-1level": (1, 10, False, 0.0, 2 * 0.0408),
    "gain-4levels": (4, 8, False, 0.0, 2 * 0.0182),
    "block-1level": (1, 24, True, HUBER_K, 2 * 0.0732),
    "block-4levels": (4, 8, True, HUBER_K, 2 * 0.0496),
}
# (row, seed) whose pair does not keep RATIO on the host reference (2.3 x: without the model this pair happens to end 0.09 px off) and is not asked to
RATIO_DROPPED = {("block-1level", 2)}


def opts(max_iterations=6, min_valid=20000, lambda0=1e-3, eps_px=1e-3, brightness=1, huber_k=10.0, gain0=1.0, bias0=0.0):
    """hnet_photo_robust_opts with the defaults of hnet_photo_robust_default_opts (no library needed)"""
    return _capi.PhotoRobustOpts(_capi.PhotoAlignOpts(max_iterations, min_valid, lambda0, eps_px), brightness, 0, huber_k, gain0, bias0)


def build_ref(tmp):
    so = str(tmp / "photo_robust_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", *U.HOST_FLAGS, os.path.join(ROOT, "tests", "cpp", "photo_robust_ref.cpp"),
                    "-o", so], check=True)
    return C.CDLL(so)


def spoil(img2, gain=GAIN, bias=BIAS, block=None, seed=0):
    """an exposure step and, with block = (row, column, rows, columns), a block of uniform noise no homography explains:
    clip(floor(gain img2 + bias + 0.5)) (round half up), then the block filled from np.random.RandomState(seed)"""
    out = np.clip(np.floor(gain * np.asarray(img2, np.float64) + bias + 0.5), 0, 255).astype(np.uint8)
    if block is not None:
        r, c, h, w = block
        out[r:r + h, c:c + w] = np.random.RandomState(seed).randint(0, 256, (h, w)).astype(np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def row_pairs(name):
    """the four pairs of an accuracy row -> (img1 [4], spoiled img2 [4], truth [4, 8], start offsets f32 [4, 8])"""
    levels, _, block, _, _ = ROWS[name]
    i1, i2, truth, start = [], [], [], []
    for seed in U.SEEDS:
        if levels == 1:
            a, b, off, s = U.stock_pair(seed)
        else:
            a, b, off = P.basin_pair(seed, 24.0)
            s = np.zeros(8, np.float32)
        i1.append(a)
        i2.append(spoil(b, GAIN, BIAS, BLOCK if block else None, seed))
        truth.append(off)
        start.append(s)
    return np.stack(i1), np.stack(i2), np.stack(truth), np.stack(start).astype(np.float32)


def row_opts(name):
    levels, K, _, k, _ = ROWS[name]
    return levels, dict(max_iterations=K, huber_k=k, brightness=1)


def worst_px(rec, truth):
    """worst-component distance of a record's offsets from the truth, px"""
    return float(np.abs(rec["px"]["offsets_px"].astype(np.float64) - truth).max())


def hostile_cases():
    """(name, img1, img2, start offsets, options, flag expected at every level or None): P.hostile_cases() with the model on and k = 10, and the
    starts of the brightness parameters at the ends of their range"""
    i1, i2, _ = U.smooth_pair(1, 2.0)
    out = [(n, a, b, s, {}, f) for n, a, b, s, f in P.hostile_cases()]
    zero = np.zeros(8, np.float32)
    out += [("gain0-1e-30", i1, i2, zero, dict(gain0=1e-30), None), ("gain0-1e30", i1, i2, zero, dict(gain0=1e30), None),
            ("all-outliers", i1, i2, zero, dict(huber_k=1e-6), None)]
    return out


def _frames(img1, img2):
    return U._frames(img1, img2)


def ref_sums(lib, img1, img2, offsets, gain, bias, k, level):
    """-> sums [n] (SUMS) of level `level` at offsets [n, 8], gain [n], bias [n] and threshold k; has-a-homography [n]"""
    a, b = _frames(img1, img2)
    n = a.shape[0]
    off = np.ascontiguousarray(offsets, np.float32).reshape(n, 8)
    G, B = np.ascontiguousarray(np.broadcast_to(gain, n), np.float64), np.ascontiguousarray(np.broadcast_to(bias, n), np.float64)
    out, ok = np.zeros(n, SUMS), np.zeros(n, np.int32)
    lib.photo_robust_ref_sums(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), n, C.c_void_p(off.ctypes.data), C.c_void_p(G.ctypes.data),
                              C.c_void_p(B.ctypes.data), C.c_double(k), int(level), C.c_void_p(out.ctypes.data), C.c_void_p(ok.ctypes.data))
    return out, ok


def ref_reduce(lib, offsets, gain, sums):
    """-> A10 [n, 10, 10], g10 [n, 10]"""
    off = np.ascontiguousarray(offsets, np.float32).reshape(-1, 8)
    n = off.shape[0]
    G = np.ascontiguousarray(np.broadcast_to(gain, n), np.float64)
    A, g = np.zeros((n, 10, 10)), np.zeros((n, 10))
    lib.photo_robust_ref_reduce(n, C.c_void_p(off.ctypes.data), C.c_void_p(G.ctypes.data), C.c_void_p(sums.ctypes.data), C.c_void_p(A.ctypes.data),
                                C.c_void_p(g.ctypes.data))
    return A, g


def ref_run(lib, img1, img2, offsets0, levels, **kw):
    """-> (records [n] of level 0, records [n, levels] indexed by level) of the host reference"""
    a, b = _frames(img1, img2)
    off = np.ascontiguousarray(offsets0, np.float32).reshape(a.shape[0], 8)
    out, lv, o = np.zeros(a.shape[0], REC), np.zeros((a.shape[0], levels), REC), opts(**kw)
    lib.photo_robust_ref_run(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), a.shape[0], C.c_void_p(off.ctypes.data), C.byref(o), int(levels),
                             C.c_void_p(out.ctypes.data), C.c_void_p(lv.ctypes.data))
    return out, lv


def ref_cost64(lib, img1, img2, p, k, level):
    """the float64 twin at p = (offsets [8], gain, bias) -> (sum rho / 2, gradient [10], n_valid, n_outliers, min | |r| - k |)"""
    a, b = _frames(img1, img2)
    p = np.ascontiguousarray(p, np.float64).reshape(10)
    cost, g, n, no, margin = C.c_double(), np.zeros(10), C.c_int32(), C.c_int32(), C.c_double()
    lib.photo_robust_ref_cost64(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(p.ctypes.data), C.c_double(k), int(level), C.byref(cost),
                                C.c_void_p(g.ctypes.data), C.byref(n), C.byref(no), C.byref(margin))
    return cost.value, g, n.value, no.value, margin.value


def describe_levels(lv, truth=None):
    """one line per level of one pair's records [levels]"""
    out = []
    for L in range(len(lv) - 1, -1, -1):
        r, x = lv[L], lv[L]["px"]
        err = "" if truth is None else f" {worst_px(r, truth):.4f} px off,"
        out.append(f"level {L}:{err} flags {x['flags']}, trials {x['trials']}, accepted {x['accepted']}, n_valid {x['n_valid0']} -> {x['n_valid']}, "
                   f"outliers {r['n_outliers0']} -> {r['n_outliers']}, cost {x['mse0']:.3f} -> {x['mse']:.3f}, gain {r['gain']:.4f}, bias {r['bias']:.3f}")
    return "\n".join(out)
