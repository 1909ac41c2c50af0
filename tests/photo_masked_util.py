"""What the CPU and the GPU tests of the masked robust alignment share (include/hnet.h hnet_op_photo_align_masked; include/hnet_photo_masked.h; DESIGN
7ae): the masks, the host reference tests/cpp/photo_masked_ref.cpp behind ctypes and the numpy restatement of the mask pyramid and its counts."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import photo_align_pyr_util as P
import photo_align_util as U
import photo_robust_util as R

ROOT = U.ROOT
REC = R.REC
H, W, SLICES, LEVELS = 224, 320, 7, 4
SPARSE_MIN_VALID = 500          # the second option set of the mask cases: low enough for the sparse masks to run (the default 20 000 stops them FEW_PIXELS)


def build_ref(tmp):
    so = str(tmp / "photo_masked_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", *U.HOST_FLAGS, os.path.join(ROOT, "tests", "cpp", "photo_masked_ref.cpp"),
                    "-o", so], check=True)
    return C.CDLL(so)


@functools.lru_cache(maxsize=None)
def masks():
    """name -> mask u8 [224, 320] (read-only), the cases of the issue without the composite's cover (keyframe_localise_util.composite)"""
    full = np.full((H, W), 255, np.uint8)
    out = {"full": full}
    m = full.copy()
    m[100, 157] = 0
    out["one-zero-byte"] = m
    for j in range(4):
        m = np.zeros((H, W), np.uint8)
        m[:, j::4] = 1 + 63 * j                    # (any non-zero byte admits)
        out[f"quad-byte-{j}"] = m
    m = np.zeros((H, W), np.uint8)
    m[H - 1, :] = 255
    m[:, W - 1] = 255
    out["last-row-and-column"] = m
    m = full.copy()
    m[:96] = 0
    out["rows-0-95-zero"] = m
    vs, us = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out["checkerboard"] = (((us + vs) & 1) * 255).astype(np.uint8)
    out["all-zero"] = np.zeros((H, W), np.uint8)
    for v in out.values():
        v.setflags(write=False)
    return out


def numpy_mask_pyramid(mask):
    """-> (levels [4] of 0 / 1 arrays, level 0 being mask != 0; n_mask [4, 7]): level L is 1 where all 4^L level-0 bytes under the pixel are non-zero"""
    lv = [(np.asarray(mask).reshape(H, W) != 0).astype(np.uint8)]
    for L in range(1, LEVELS):
        s = 1 << L
        lv.append(lv[0].reshape(H // s, s, W // s, s).min(axis=(1, 3)))
    n = np.array([[int(lv[L][k * (H >> L) // SLICES:(k + 1) * (H >> L) // SLICES].sum()) for k in range(SLICES)] for L in range(LEVELS)], np.int32)
    return lv, n


def ref_pyramid(lib, mask):
    """-> (packed levels 1 .. 3 [n, PYR_BYTES], n_mask [n, 4, 7]) of the host header"""
    m = np.ascontiguousarray(mask, np.uint8).reshape(-1, H, W)
    pyr, n_mask = np.full((m.shape[0], P.PYR_BYTES), 0xA5, np.uint8), np.full((m.shape[0], LEVELS, SLICES), -1, np.int32)
    lib.photo_masked_ref_pyramid(C.c_void_p(m.ctypes.data), m.shape[0], C.c_void_p(pyr.ctypes.data), C.c_void_p(n_mask.ctypes.data))
    return pyr, n_mask


def ref_run(lib, img1, mask, img2, offsets0, levels, **kw):
    """-> (records [n] of level 0, records [n, levels] indexed by level) of the host reference"""
    a, b = U._frames(img1, img2)
    m = np.ascontiguousarray(mask, np.uint8).reshape(-1, H, W)
    assert m.shape == a.shape
    off = np.ascontiguousarray(offsets0, np.float32).reshape(a.shape[0], 8)
    out, lv, o = np.zeros(a.shape[0], REC), np.zeros((a.shape[0], levels), REC), R.opts(**kw)
    lib.photo_masked_ref_run(C.c_void_p(a.ctypes.data), C.c_void_p(m.ctypes.data), C.c_void_p(b.ctypes.data), a.shape[0], C.c_void_p(off.ctypes.data), C.byref(o),
                             int(levels), C.c_void_p(out.ctypes.data), C.c_void_p(lv.ctypes.data))
    return out, lv


def scramble_under(img1, mask, seed=7):
    """img1 with every byte under a zero mask byte replaced by noise"""
    noise = np.random.RandomState(seed).randint(0, 256, (H, W)).astype(np.uint8)
    return np.where(np.asarray(mask) != 0, img1, noise).astype(np.uint8)


def trace(r):
    """every integer of a record"""
    x = r["px"]
    return (int(x["flags"]), int(x["trials"]), int(x["accepted"]), int(x["n_valid0"]), int(x["n_valid"]), int(r["n_outliers0"]), int(r["n_outliers"]))
