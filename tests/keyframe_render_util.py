"""What the CPU and the GPU tests of the keyframe render share (include/hnet.h hnet_op_keyframe_render, hnet_sessions_keyframe_render): the
host reference tests/cpp/keyframe_render_ref.cpp behind ctypes, the maps and views of the bit-for-bit cases, and the three keyframes cut from one texture
whose seam statistics the rank tests read.  Geometry helpers are keyframe_util's."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import keyframe_util as K
import photo_align_util as U
from cuahn_vio_amd import _capi, synth

ENTRY, REC = _capi.KEYFRAME_MAP_ENTRY_DTYPE, _capi.KEYFRAME_RENDER_DTYPE
MODES = (_capi.RENDER_FEWEST_LINKS, _capi.RENDER_NEWEST, _capi.RENDER_MEAN)
H, W = synth.IMG_H, synth.IMG_W


def build_ref(tmp):
    so = str(tmp / "keyframe_render_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", *U.HOST_FLAGS, os.path.join(K.ROOT, "tests", "cpp", "keyframe_render_ref.cpp"),
                    "-o", so], check=True)
    return C.CDLL(so)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def shift(dx, dy):
    return np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])


def entries(hs, links=None, serials=None, valid=None):
    """-> [m] ENTRY with h_origin_key = hs[j]; links default j, serial default j + 1, valid default 1"""
    m = len(hs)
    e = np.zeros(m, ENTRY)
    for j in range(m):
        e[j]["valid"] = 1 if valid is None else valid[j]
        e[j]["links"] = j if links is None else links[j]
        e[j]["serial"] = j + 1 if serials is None else serials[j]
        e[j]["h_origin_key"] = hs[j]
    return e


def ref_setup(lib, view, entry):
    """-> S [3, 3] or None"""
    v, e, s = np.ascontiguousarray(view, np.float64).reshape(3, 3), np.ascontiguousarray(entry, ENTRY).reshape(1), np.zeros((3, 3))
    return s if lib.keyframe_render_ref_setup(_p(v), _p(e), _p(s)) else None


def ref_sample(lib, s, img, u, v):
    """-> the byte or None"""
    s, img, val = np.ascontiguousarray(s, np.float64).reshape(3, 3), np.ascontiguousarray(img, np.uint8).reshape(H, W), C.c_uint8(0)
    return int(val.value) if lib.keyframe_render_ref_sample(_p(s), _p(img), int(u), int(v), C.byref(val)) else None


def ref_pixel(lib, vals, mask, links, serials, mode):
    """one pixel from its samples -> (out, cover, n [8], sse [8])"""
    v = np.zeros(8, np.uint8)
    v[:len(vals)] = vals
    li, se = np.zeros(8, np.int32), np.zeros(8, np.int32)
    li[:len(links)], se[:len(serials)] = links, serials
    n, sse, cover = np.zeros(8, np.uint64), np.zeros(8, np.uint64), C.c_int(-1)
    out = lib.keyframe_render_ref_pixel(_p(v), int(mask), _p(li), _p(se), int(mode), C.byref(cover), _p(n), _p(sse))
    return int(out), int(cover.value), n, sse


def ref_fit_view(lib, ent, width, height, margin):
    e, h = np.ascontiguousarray(ent, ENTRY).reshape(-1), np.full((3, 3), -7.0)
    return h if lib.keyframe_render_ref_fit_view(_p(e), len(e), int(width), int(height), C.c_double(margin), _p(h)) else None


def ref_render(lib, images, ent, view, width, height, mode):
    """the host reference's whole render -> (image [height, width], cover [height, width], record [1] REC)"""
    img, e = np.ascontiguousarray(images, np.uint8).reshape(-1, H, W), np.ascontiguousarray(ent, ENTRY).reshape(-1)
    assert len(e) == img.shape[0]
    v, o = np.ascontiguousarray(view, np.float64).reshape(3, 3), _capi.KeyframeRenderOpts(int(width), int(height), int(mode), 0)
    out, cover, rec = np.full((height, width), 0xA5, np.uint8), np.full((height, width), 0xA5, np.uint8), np.zeros(1, REC)
    rec.view(np.uint8)[:] = 0xA5                                           # every byte must be written
    lib.keyframe_render_ref_render(len(e), _p(img), _p(e), _p(v), C.byref(o), _p(out), _p(cover), _p(rec))
    return out, cover, rec


# ---- the maps of the bit-for-bit cases: m frames of one canvas at poses up to 40 px off, h_origin_key = H(pose)

@functools.lru_cache(maxsize=None)
def pose_map(m, seed=3):
    """-> (images u8 [m, 224, 320], entries [m]); entry j has links (3 j) % 5 and serial m - j, so that the three modes pick differently"""
    cv = synth.canvas(seed)
    poses = [np.zeros(8)] + [synth.true_offsets(seed * 10 + j, 40.0) for j in range(1, m)]
    images = np.stack([K.render(cv, p) for p in poses])
    e = entries([K.homography(p) for p in poses], links=[(3 * j) % 5 for j in range(m)], serials=[m - j for j in range(m)])
    images.setflags(write=False)
    e.setflags(write=False)
    return images, e


# The views of the bit-for-bit cases: (width, height) -> h_origin_view.  320 x 224: the origin frame turned by 0.1 rad about its centre with a little
# perspective, so that the taps cross rows and columns; 50 x 37 (no multiple of any tile): the origin frame scaled down by 6 and shifted, parts of it
# outside every keyframe; 1 x 1: one pixel at a fractional position; 1 x 300: one column, taller than the keyframes, that leaves them at both ends
def view(width, height):
    if (width, height) == (320, 224):
        c, s = np.cos(0.1), np.sin(0.1)
        r = np.array([[c, -s, 0.0], [s, c, 0.0], [1e-5, -2e-5, 1.0]])
        return shift(159.5, 111.5) @ r @ shift(-159.5, -111.5)
    if (width, height) == (50, 37):
        return np.array([[1 / 6.0, 0.0, 3.25], [0.0, 1 / 6.0, -2.5], [0.0, 0.0, 1.0]])
    if (width, height) == (1, 1):
        return shift(-100.3, -80.7)
    if (width, height) == (1, 300):
        return np.array([[1.0, 0.0, -150.5], [0.0, 0.9, 11.0], [0.0, 0.0, 1.0]])
    raise KeyError((width, height))


VIEWS = ((320, 224), (50, 37), (1, 1), (1, 300))


# ---- three keyframes cut from one texture by known homographies, and the same map with entry 1's matrix displaced by 2 px

DISPLACED = 1


@functools.lru_cache(maxsize=None)
def texture_map(seed=7):
    """-> (images [3], exact entries [3], entries with h_origin_key[DISPLACED] displaced by 2 px in x): frames of synth.canvas(seed) at the poses 0,
    (+30, +12) px with a little warp, and synth.true_offsets(seed, 25)"""
    cv = synth.canvas(seed)
    poses = [np.zeros(8), np.tile([30.0, 12.0], 4) + synth.true_offsets(seed + 1, 3.0), synth.true_offsets(seed, 25.0)]
    images = np.stack([K.render(cv, p) for p in poses])
    hs = [K.homography(p) for p in poses]
    exact = entries(hs)
    off = entries([shift(2.0, 0.0) @ h if j == DISPLACED else h for j, h in enumerate(hs)])
    for a in (images, exact, off):
        a.setflags(write=False)
    return images, exact, off


def seam_mse(rec):
    """sse[j] / n[j] of the first three slots of a record"""
    r = np.asarray(rec).reshape(-1)[0]
    assert (r["n"][:3] > 0).all()
    return r["sse"][:3].astype(np.float64) / r["n"][:3].astype(np.float64)


def check_ranks(exact_rec, off_rec):
    """the inequalities of the texture map: every entry disagrees less with exact matrices than with one displaced, and the displaced entry most"""
    a, b = seam_mse(exact_rec), seam_mse(off_rec)
    print("sse / n exact", a, "displaced", b)
    assert (a < b).all()
    assert int(np.argmax(b)) == DISPLACED
