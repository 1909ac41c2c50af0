"""The wide canvas and the composite cases of DESIGN 7ae (a camera between stored keyframes, aligned against the rendered map through
hnet_op_photo_align_masked): a canvas with a 240 px border, keyframes cut from it at known poses, the camera's frame, the view the chain predicts and the
composite / cover of the keyframes in that view by the keyframe render's host reference.  synth.py stays as it is: the canvas is built from its octaves."""
import functools

import numpy as np

import keyframe_render_util as KR
import keyframe_util as K
from cuahn_vio_amd import _capi, synth

PAD = 240                                   # the border of the wide canvas (synth._PAD is 48)
SEEDS = (1, 2, 5, 11)
LEVELS, TRIALS = 3, 6
# the composite rows: name -> (keyframe centres (x, y) px, drift px of the predicted view)
ROWS = {
    "two-keyframes-drift8": (((-200.0, 0.0), (200.0, 0.0)), 8.0),
    "two-keyframes-drift0": (((-200.0, 0.0), (200.0, 0.0)), 0.0),
    "four-keyframes-drift8": (((-140.0, -100.0), (140.0, -100.0), (-140.0, 100.0), (140.0, 100.0)), 8.0),
}
# The gate of a row is TWICE the worst distance from the truth (worst corner component, px) of the host reference tests/cpp/photo_masked_ref.cpp over SEEDS, as
# tests/test_photo_masked_cpu.py::test_composite_rows prints it (DESIGN 7ae holds the measured values)
GATES = {"two-keyframes-drift8": 2 * 0.0123, "two-keyframes-drift0": 2 * 0.0522, "four-keyframes-drift8": 2 * 0.0100}
MASKED_MSE_BELOW, UNMASKED_MSE_ABOVE = 10.0, 100.0        # the two-keyframe rows: the mean robust cost with and without the mask on the same composite
BEFORE_GATES = 3.0                                         # every drift-8 start lies at least this many gates from the truth


@functools.lru_cache(maxsize=None)
def wide_canvas(seed):
    """int64 texture in [0, 255], [224 + 2 PAD, 320 + 2 PAD]: photo_align_util.smooth_pair's octaves (32-, 16- and 8-pixel cells, 4 : 3 : 2), stretched"""
    h, w = synth.IMG_H + 2 * PAD, synth.IMG_W + 2 * PAD
    t = 4 * synth._octave(h, w, 5, seed * 4 + 1) + 3 * synth._octave(h, w, 4, seed * 4 + 2) + 2 * synth._octave(h, w, 3, seed * 4 + 3)
    t = t // 9
    lo, hi = int(t.min()), int(t.max())
    return ((t - lo) * 255) // max(hi - lo, 1)


def render(cv, pose):
    """keyframe_util.render on the wide canvas: frame(q) = scene(H(pose)^-1 q)"""
    hinv = np.linalg.inv(K.homography(pose))
    vs, us = np.meshgrid(np.arange(synth.IMG_H, dtype=np.float64), np.arange(synth.IMG_W, dtype=np.float64), indexing="ij")
    xw = hinv[0, 0] * us + hinv[0, 1] * vs + hinv[0, 2]
    yw = hinv[1, 0] * us + hinv[1, 1] * vs + hinv[1, 2]
    zw = hinv[2, 0] * us + hinv[2, 1] * vs + hinv[2, 2]
    img = np.floor(synth._bilinear(cv, xw / zw + PAD, yw / zw + PAD) + 0.5)
    return np.clip(img, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scene(name, seed):
    """-> dict: images [m] of the keyframes, their entries [m] (exact h_origin_key, links 1 + j), cam_pose / pred_pose [8], the camera's frame, the view
    h_origin_pred [3, 3] and truth [8]: the offsets predicted view -> current frame the alignment should find.  A keyframe's pose is its centre (a camera
    at (x, y) sees the scene shifted by (-x, -y)) plus up to 3 px of warp; the camera sits at synth.true_offsets(seed + 100, 6); the prediction is off by
    synth.true_offsets(seed + 200, drift)."""
    centres, drift = ROWS[name]
    cv = wide_canvas(seed)
    poses = [np.tile([-x, -y], 4) + synth.true_offsets(seed * 10 + j, 3.0) for j, (x, y) in enumerate(centres)]
    cam = synth.true_offsets(seed + 100, 6.0)
    pred = cam + synth.true_offsets(seed + 200, drift) if drift > 0.0 else cam.copy()
    out = dict(images=np.stack([render(cv, p) for p in poses]), entries=KR.entries([K.homography(p) for p in poses], links=[1 + j for j in range(len(poses))]),
               cam_pose=cam, pred_pose=pred, frame=render(cv, cam), view=K.homography(pred), truth=K.relative(pred, cam))
    for v in out.values():
        v.setflags(write=False)
    return out


def composite(render_lib, name, seed):
    """the FEWEST_LINKS composite and cover [224, 320] of a scene's keyframes in its predicted view, and the render's record, by the host reference"""
    s = scene(name, seed)
    return KR.ref_render(render_lib, s["images"], s["entries"], s["view"], synth.IMG_W, synth.IMG_H, _capi.RENDER_FEWEST_LINKS)


MIN_GRID = 32                                              # hnet_keyframe_revisit_default_opts: what the revisit's select asks of ONE stored keyframe


def revisit_select(name, seed):
    """what the existing revisit sees of a scene from its predicted view (keyframe_map_util's numpy select, every valid entry eligible)
    -> (slot or -1 of np_select with min_grid = MIN_GRID, the grid count of every entry)"""
    import keyframe_map_util as KM
    s = scene(name, seed)
    grids = []
    for e in s["entries"]:
        r = KM.np_relative(s["view"], e["h_origin_key"])
        grids.append(-1 if r is None else KM.np_grid_count(r[0]))
    slot = KM.np_select(dict(cur_slot=-1, cur_links=1 << 30), s["entries"], s["view"], MIN_GRID)[0]
    return slot, grids


def worst_corner_px(offsets, truth):
    return float(np.abs(np.asarray(offsets, np.float64) - truth).max())


# ---- the localise rule (include/hnet_keyframe_localise.h) behind ctypes: tests/cpp/keyframe_localise_ref.cpp

LOCALISE = _capi.KEYFRAME_LOCALISE_DTYPE


def loc_opts(levels=LEVELS, mode=_capi.RENDER_FEWEST_LINKS, min_cover=0.5, min_overlap=0.4, max_mse=0.0, max_shift_px=0.0, apply=0, **align):
    """hnet_keyframe_localise_opts with the defaults of hnet_keyframe_localise_default_opts and 6 trials (no library needed)"""
    import photo_robust_util as R
    a = dict(max_iterations=TRIALS)
    a.update(align)
    return _capi.KeyframeLocaliseOpts(R.opts(**a), levels, mode, min_cover, min_overlap, max_mse, max_shift_px, apply, 0)


def build_rule_ref(tmp):
    import ctypes as C
    import os
    import subprocess
    import photo_align_util as U
    so = str(tmp / "keyframe_localise_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", *U.HOST_FLAGS, os.path.join(K.ROOT, "tests", "cpp", "keyframe_localise_ref.cpp"),
                    "-o", so], check=True)
    return C.CDLL(so)


def _p(a):
    import ctypes as C
    return None if a is None else C.c_void_p(a.ctypes.data)


def ref_start(lib, used_mask, n_covered, o):
    import ctypes as C
    x0 = np.full(8, 7.0, np.float32)
    lib.keyframe_localise_ref_start(int(used_mask), C.c_uint64(int(n_covered)), C.byref(o), _p(x0))
    return x0


def ref_eligible_mask(lib, mstate, entries):
    e = np.ascontiguousarray(entries, KR.ENTRY).reshape(-1)
    return int(lib.keyframe_localise_ref_eligible_mask(_p(mstate), _p(e), len(e)))


def ref_decide(lib, state, mstate, entries, used_mask, n_covered, h_before, rec, o):
    """the header's decide_localise -> (localised 0 / 1, record [1] LOCALISE with rec copied in, new state, new map state, new entries); state and mstate
    None together: the operator-level call (the new states are None)"""
    import ctypes as C
    import keyframe_map_util as KM
    e = np.ascontiguousarray(entries, KR.ENTRY).reshape(-1)
    hb, r = np.ascontiguousarray(h_before, np.float64).reshape(3, 3), np.ascontiguousarray(rec, _capi.PHOTO_ROBUST_DTYPE).reshape(1)
    out = np.zeros(1, LOCALISE)
    out.view(np.uint8)[:] = 0xA5                                           # every byte must be written
    ns = nm = None
    ne = e.copy()
    ne.view(np.uint8)[:] = 0xA5
    if state is not None:
        state, mstate = np.ascontiguousarray(state, K.STATE).reshape(1), np.ascontiguousarray(mstate, KM.MSTATE).reshape(1)
        ns, nm = np.zeros(1, K.STATE), np.zeros(1, KM.MSTATE)
    got = lib.keyframe_localise_ref_decide(_p(state), _p(mstate), _p(e), len(e), int(used_mask), C.c_uint64(int(n_covered)), _p(hb), _p(r), C.byref(o), _p(ns), _p(nm),
                                           _p(ne), _p(out))
    return int(got), out, ns, nm, ne
