"""What the CPU and the GPU tests of photometric alignment share (include/hnet.h hnet_photo_align): the test pairs, the host reference
tests/cpp/photo_align_ref.cpp behind ctypes, and the record layouts."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from cuahn_vio_amd import _capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPIX = 224 * 320
SEEDS = (1, 2, 5, 11)
CONVERGED, SINGULAR, DEGENERATE, FEW_PIXELS = 1, 2, 4, 8
HOST_FLAGS = ["-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "cuahn_vio_amd", "csrc"),
              "-I", os.path.join(ROOT, "include")]
# hnet_photo_align (656 bytes) and hnet_align::Sums (448 bytes)
REC = _capi.PHOTO_ALIGN_DTYPE
SUMS = np.dtype([("ss", "<f8", 45), ("sr", "<f8", 9), ("rr", "<f8"), ("n_valid", "<i4"), ("pad", "<i4")])
assert REC.itemsize == 656 and SUMS.itemsize == 448


def opts(max_iterations=6, min_valid=20000, lambda0=1e-3, eps_px=1e-3):
    """hnet_photo_align_opts with the defaults of hnet_photo_align_default_opts (no library needed)"""
    return _capi.PhotoAlignOpts(max_iterations, min_valid, lambda0, eps_px)


@functools.lru_cache(maxsize=None)
def smooth_pair(seed, max_offset):
    """a pair whose texture has no cell finer than 8 pixels: synth.canvas's octaves of 32-, 16- and 8-pixel cells weighted 4 : 3 : 2, contrast-stretched
    and warped exactly as synth.make_pair does -> (img1 u8, img2 u8, true offsets f64 [8])"""
    pad = synth._PAD
    h, w = synth.IMG_H + 2 * pad, synth.IMG_W + 2 * pad
    t = 4 * synth._octave(h, w, 5, seed * 4 + 1) + 3 * synth._octave(h, w, 4, seed * 4 + 2) + 2 * synth._octave(h, w, 3, seed * 4 + 3)
    t = t // 9
    lo, hi = int(t.min()), int(t.max())
    cv = ((t - lo) * 255) // max(hi - lo, 1)
    img1 = cv[pad:pad + synth.IMG_H, pad:pad + synth.IMG_W].astype(np.uint8)
    off = synth.true_offsets(seed, max_offset)
    hinv = np.linalg.inv(synth.dlt_h(off))
    vs, us = np.meshgrid(np.arange(synth.IMG_H, dtype=np.float64), np.arange(synth.IMG_W, dtype=np.float64), indexing="ij")
    xw = hinv[0, 0] * us + hinv[0, 1] * vs + hinv[0, 2]
    yw = hinv[1, 0] * us + hinv[1, 1] * vs + hinv[1, 2]
    zw = hinv[2, 0] * us + hinv[2, 1] * vs + hinv[2, 2]
    img2 = np.floor(synth._bilinear(cv, xw / zw + pad, yw / zw + pad) + 0.5)
    return img1, np.clip(img2, 0, 255).astype(np.uint8), off


@functools.lru_cache(maxsize=None)
def stock_pair(seed):
    """synth.make_pair(seed, 12.0) and its sigma = 1 prior -> (img1, img2, true offsets, start offsets f32)"""
    i1, i2, off = synth.make_pair(seed, 12.0)
    return i1, i2, off, synth.make_prior(seed, off, 1.0)


def convergence_cases():
    """the pairs of the convergence tests: (name, img1, img2, truth, start offsets, gate in px)"""
    out = []
    for seed in SEEDS:
        for mo in (2.0, 8.0):
            i1, i2, off = smooth_pair(seed, mo)
            out.append((f"smooth{int(mo)}-{seed}", i1, i2, off, np.zeros(8, np.float32), 0.05))
        i1, i2, off, start = stock_pair(seed)
        out.append((f"stock-{seed}", i1, i2, off, start, 0.1))
    return out


def degenerate_cases():
    """(name, img1, img2, start offsets, flag expected, info exactly zero)"""
    i1, i2, _ = smooth_pair(1, 2.0)
    const = np.full((224, 320), 93, np.uint8)
    stripes = np.tile(i2[100:101], (224, 1))
    p4 = np.array([0, 0, 0, 223, 319, 223, 319, 0], np.float32)
    line = np.array([0, 0, 10, 5, 20, 10, 30, 15], np.float32) - p4            # all four corners on one line: det = 0
    far = np.tile(np.array([400.0, 0.0], np.float32), 4)
    zero = np.zeros(8, np.float32)
    return [("constant", i1, const, zero, SINGULAR, True), ("stripes", i1, stripes, zero, SINGULAR, False),
            ("no-homography", i1, i2, line, DEGENERATE, True), ("far", i1, i2, far, FEW_PIXELS, True)]


def build_ref(tmp):
    so = str(tmp / "photo_align_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", *HOST_FLAGS, os.path.join(ROOT, "tests", "cpp", "photo_align_ref.cpp"),
                    "-o", so], check=True)
    return C.CDLL(so)


def _frames(img1, img2):
    a = np.ascontiguousarray(img1, np.uint8).reshape(-1, 224, 320)
    b = np.ascontiguousarray(img2, np.uint8).reshape(-1, 224, 320)
    assert a.shape == b.shape
    return a, b


def ref_sums(lib, img1, img2, offsets):
    """-> H-space sums [n] (SUMS), has-a-homography [n]"""
    a, b = _frames(img1, img2)
    off = np.ascontiguousarray(offsets, np.float32).reshape(a.shape[0], 8)
    out, ok = np.zeros(a.shape[0], SUMS), np.zeros(a.shape[0], np.int32)
    lib.photo_align_ref_sums(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), a.shape[0], C.c_void_p(off.ctypes.data), C.c_void_p(out.ctypes.data),
                             C.c_void_p(ok.ctypes.data))
    return out, ok


def ref_reduce(lib, offsets, sums):
    """-> A [n, 8, 8], g [n, 8]"""
    off = np.ascontiguousarray(offsets, np.float32).reshape(-1, 8)
    A, g = np.zeros((off.shape[0], 8, 8)), np.zeros((off.shape[0], 8))
    lib.photo_align_ref_reduce(off.shape[0], C.c_void_p(off.ctypes.data), C.c_void_p(sums.ctypes.data), C.c_void_p(A.ctypes.data), C.c_void_p(g.ctypes.data))
    return A, g


def ref_run(lib, img1, img2, offsets0, **kw):
    """-> records [n] (REC) of the host reference's alignment"""
    a, b = _frames(img1, img2)
    off = np.ascontiguousarray(offsets0, np.float32).reshape(a.shape[0], 8)
    out, o = np.zeros(a.shape[0], REC), opts(**kw)
    lib.photo_align_ref_run(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), a.shape[0], C.c_void_p(off.ctypes.data), C.byref(o), C.c_void_p(out.ctypes.data))
    return out


def ref_cost64(lib, img1, img2, offsets):
    """the float64 twin -> (sum r^2 / 2, gradient [8], n_valid)"""
    a, b = _frames(img1, img2)
    off = np.ascontiguousarray(offsets, np.float64).reshape(8)
    cost, g, n = C.c_double(), np.zeros(8), C.c_int32()
    lib.photo_align_ref_cost64(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(off.ctypes.data), C.byref(cost), C.c_void_p(g.ctypes.data),
                               C.byref(n))
    return cost.value, g, n.value
