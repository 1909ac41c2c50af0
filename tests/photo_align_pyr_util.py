"""What the CPU and the GPU tests of coarse-to-fine photometric alignment share (include/hnet.h hnet_op_photo_align_pyramid): the basin and
the hostile cases, the host reference tests/cpp/photo_align_pyr_ref.cpp behind ctypes, and a numpy restatement of the pyramid."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import photo_align_util as U
from cuahn_vio_amd import synth

ROOT = U.ROOT
MAX_LEVELS = 4
LEVEL_W, LEVEL_H = (320, 160, 80, 40), (224, 112, 56, 28)
LEVEL_OFFSET = (None, 0, 17920, 22400)
PYR_BYTES = 17920 + 4480 + 1120


def build_ref(tmp):
    so = str(tmp / "photo_align_pyr_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", *U.HOST_FLAGS,
                    os.path.join(ROOT, "tests", "cpp", "photo_align_pyr_ref.cpp"), "-o", so], check=True)
    return C.CDLL(so)


def numpy_pyramid(img):
    """levels 1 .. 3 of one u8 frame [224, 320] -> [lvl1, lvl2, lvl3]: (a + b + c + d + 2) >> 2 over 2 x 2 blocks, cascaded"""
    out, cur = [], np.asarray(img, np.uint8)
    for _ in range(3):
        w = cur.astype(np.uint32)
        cur = ((w[0::2, 0::2] + w[0::2, 1::2] + w[1::2, 0::2] + w[1::2, 1::2] + 2) >> 2).astype(np.uint8)
        out.append(cur)
    return out


def split_pyramid(packed):
    """packed [PYR_BYTES] u8 -> [lvl1 [112, 160], lvl2 [56, 80], lvl3 [28, 40]]"""
    p = np.asarray(packed, np.uint8).reshape(PYR_BYTES)
    return [p[LEVEL_OFFSET[L]:LEVEL_OFFSET[L] + LEVEL_W[L] * LEVEL_H[L]].reshape(LEVEL_H[L], LEVEL_W[L]) for L in (1, 2, 3)]


def ref_pyramid(lib, img):
    """-> packed levels 1 .. 3 [n, PYR_BYTES]"""
    a = np.ascontiguousarray(img, np.uint8).reshape(-1, 224, 320)
    out = np.zeros((a.shape[0], PYR_BYTES), np.uint8)
    lib.photo_align_pyr_ref_pyramid(C.c_void_p(a.ctypes.data), a.shape[0], C.c_void_p(out.ctypes.data))
    return out


def ref_sums(lib, img1, img2, offsets, level):
    """-> H-space sums [n] (U.SUMS) of level `level`, has-a-homography [n]"""
    a, b = U._frames(img1, img2)
    off = np.ascontiguousarray(offsets, np.float32).reshape(a.shape[0], 8)
    out, ok = np.zeros(a.shape[0], U.SUMS), np.zeros(a.shape[0], np.int32)
    lib.photo_align_pyr_ref_sums(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), a.shape[0], C.c_void_p(off.ctypes.data), int(level),
                                 C.c_void_p(out.ctypes.data), C.c_void_p(ok.ctypes.data))
    return out, ok


def ref_run(lib, img1, img2, offsets0, levels, **kw):
    """-> (records [n] of level 0, records [n, levels] indexed by level) of the host reference"""
    a, b = U._frames(img1, img2)
    off = np.ascontiguousarray(offsets0, np.float32).reshape(a.shape[0], 8)
    out, lv, o = np.zeros(a.shape[0], U.REC), np.zeros((a.shape[0], levels), U.REC), U.opts(**kw)
    lib.photo_align_pyr_ref_run(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), a.shape[0], C.c_void_p(off.ctypes.data), C.byref(o), int(levels),
                                C.c_void_p(out.ctypes.data), C.c_void_p(lv.ctypes.data))
    return out, lv


def ref_cost64(lib, img1, img2, offsets, level):
    """the float64 twin of level `level` -> (sum r^2 / 2, gradient [8], n_valid)"""
    a, b = U._frames(img1, img2)
    off = np.ascontiguousarray(offsets, np.float64).reshape(8)
    cost, g, n = C.c_double(), np.zeros(8), C.c_int32()
    lib.photo_align_pyr_ref_cost64(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(off.ctypes.data), int(level), C.byref(cost),
                                   C.c_void_p(g.ctypes.data), C.byref(n))
    return cost.value, g, n.value


@functools.lru_cache(maxsize=None)
def basin_pair(seed, max_offset):
    """synth.make_pair(seed, max_offset) -> (img1, img2, true offsets f64 [8]); aligned from zero offsets"""
    return synth.make_pair(seed, float(max_offset))


def basin_cases(max_offset=32.0):
    """-> (img1 [4], img2 [4], truth [4, 8]) of seeds 1, 2, 5, 11"""
    ps = [basin_pair(s, max_offset) for s in U.SEEDS]
    return np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps]), np.stack([p[2] for p in ps])


def nan_start():
    """a quiet NaN with a payload in component 3, zeros elsewhere"""
    x = np.zeros(8, np.float32)
    x.view(np.uint32)[3] = 0x7FC12345
    return x


def hostile_cases():
    """U.degenerate_cases() and a NaN start: (name, img1, img2, start offsets, flag expected at every level)"""
    i1, i2, _ = U.smooth_pair(1, 2.0)
    return [(n, a, b, s, f) for n, a, b, s, f, _z in U.degenerate_cases()] + [("nan", i1, i2, nan_start(), U.DEGENERATE)]


def describe_levels(lv, truth=None):
    """one line per level of one pair's records [levels]"""
    out = []
    for L in range(len(lv) - 1, -1, -1):
        r = lv[L]
        err = "" if truth is None else f" {np.abs(r['offsets_px'].astype(np.float64) - truth).max():.4f} px off,"
        out.append(f"level {L}:{err} flags {r['flags']}, trials {r['trials']}, accepted {r['accepted']}, n_valid {r['n_valid0']} -> {r['n_valid']}, "
                   f"mse {r['mse0']:.3f} -> {r['mse']:.3f}")
    return "\n".join(out)
