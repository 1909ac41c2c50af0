"""What the CPU and the GPU tests of tracking against a held keyframe share (include/hnet.h hnet_sessions_keyframe_track): frame sequences
rendered from synth.canvas under a list of true homographies, the two accuracy rows and their gates, the host reference tests/cpp/keyframe_ref.cpp
behind ctypes, a numpy float64 restatement of the rule, and the record layouts."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import photo_align_util as U
from cuahn_vio_amd import _capi, synth

ROOT = U.ROOT
TRACK = _capi.KEYFRAME_TRACK_DTYPE
REC = _capi.PHOTO_ROBUST_DTYPE
STATE = np.dtype([("has_key", "<i4"), ("age", "<i4"), ("keyframes", "<i4"), ("pad", "<i4"), ("key_px", "<f4", 8), ("h_origin_key", "<f8", (3, 3))])
assert TRACK.itemsize == 1720 and STATE.itemsize == 120
NPIX = 224 * 320
P4 = synth.P4.reshape(8)
LEVELS, TRIALS = 3, 6                      # the options of every test: levels = 3, 6 trials
STEP_SIGMA = 0.3                           # px: the pseudo-noise on the steps (synth.make_prior)

# The accuracy rows: name -> (rekey_overlap, gate on key_px in px, gate on the corners of h_origin_curr in px).  A gate is TWICE the worst distance from the
# truth (worst component, px) of the host reference over seeds 1, 2, 5, 11 and every frame of the row, as tests/test_keyframe_cpu.py::test_accuracy_rows
# prints it (DESIGN 7p holds the measured values)
ROWS = {
    "out-and-back": (0.6, 2 * 0.0815, 2 * 0.0815),
    "translation-32": (0.9, 2 * 3.55e-5, 2 * 5.29e-5),
}
DRIFT_RATIO = 3.0                          # the chained sum of the noisy steps must end at least this many gates off at frame 8 of out-and-back


def opts(levels=LEVELS, auto_rekey=1, max_age=0, rekey_overlap=0.6, max_mse=0.0, **align):
    """hnet_keyframe_opts with the defaults of hnet_keyframe_default_opts and 6 trials (no library needed)"""
    a = dict(max_iterations=TRIALS)
    a.update(align)
    import photo_robust_util as R
    return _capi.KeyframeOpts(R.opts(**a), levels, auto_rekey, max_age, 0, rekey_overlap, max_mse)


def opts_kw(o):
    """the keyword form of `o` for HnetSessions.keyframe_track"""
    return dict(max_iterations=o.align.base.max_iterations, min_valid=o.align.base.min_valid, lambda0=o.align.base.lambda0, eps_px=o.align.base.eps_px,
                brightness=o.align.brightness, huber_k=o.align.huber_k, gain0=o.align.gain0, bias0=o.align.bias0, levels=o.levels, auto_rekey=o.auto_rekey,
                max_age=o.max_age, rekey_overlap=o.rekey_overlap, max_mse=o.max_mse)


# ---- geometry in float64 (numpy): the restatement the header is tested against

def homography(x):
    """H(x), h[8] = 1: the 8 x 8 linear system of the DLT solved by numpy"""
    return synth.dlt_h(np.asarray(x, np.float64))


def corners(h):
    """the image corners under h, minus the corners -> offsets [8] f64"""
    p = synth.P4
    q = np.concatenate([p, np.ones((4, 1))], axis=1) @ np.asarray(h, np.float64).reshape(3, 3).T
    return (q[:, :2] / q[:, 2:3] - p).reshape(8)


def np_compose(step, key):
    """-> offsets [8] f64 of H(step) . H(key), unrounded"""
    return corners(homography(step) @ homography(key))


def np_decide(s, start, rec, o, gap):
    """the rule of include/hnet_keyframe.h restated -> (new state dict, output dict, copy); s: dict(has_key, age, keyframes, key_px, h_origin_key)"""
    eye = np.eye(3)
    if not s["has_key"]:
        ns = dict(has_key=1, age=0, keyframes=1, key_px=np.zeros(8, np.float32), h_origin_key=eye)
        return ns, dict(start_px=np.zeros(8, np.float32), key_px=np.zeros(8, np.float32), h_origin_curr=eye, overlap=0.0, age=0, keyframes=1,
                        flags=_capi.KF_FIRST | _capi.KF_REKEYED), 1
    flags = _capi.KF_GAP if gap else 0
    age, keyframes = s["age"] + 1, s["keyframes"]
    start = np.asarray(start, np.float32)
    x = rec["px"]["offsets_px"]
    why = 0
    if not np.isfinite(start).all():
        why = _capi.KF_NO_START
    elif rec["px"]["flags"] & (U.SINGULAR | U.DEGENERATE | U.FEW_PIXELS):
        why = _capi.KF_STOPPED
    elif o.max_mse > 0 and not rec["px"]["mse"] <= o.max_mse:
        why = _capi.KF_MSE_ABOVE_MAX
    elif not np.isfinite(x).all():
        why = _capi.KF_NON_FINITE
    flags |= why

    def usable(v):
        if not np.isfinite(v).all():
            return None
        try:
            h = homography(v)
        except np.linalg.LinAlgError:
            return None
        return h if np.isfinite(h).all() else None

    if why:
        hx = usable(start)
        if hx is not None:
            key = start.copy()
            flags |= _capi.KF_BRIDGED
        else:
            key = s["key_px"].copy()
            hx = usable(key)
            if o.auto_rekey and hx is not None:
                flags |= _capi.KF_BRIDGED
    else:
        key = x.copy()
        hx = usable(key)

    def chain(a, b):
        with np.errstate(invalid="ignore"):
            m = a @ b
        if not np.isfinite(m).all() or abs(m[2, 2]) < 1e-12 * np.abs(m).max():
            return None
        return m / m[2, 2]

    ho = s["h_origin_key"]
    hc = chain(hx, ho) if hx is not None else None
    if hc is None:
        flags |= _capi.KF_ORIGIN_RESTARTED
        ho = eye
        hc = chain(hx, ho) if hx is not None else None
        if hc is None:
            hc = eye
    overlap = float(rec["px"]["n_valid"]) / 71680.0
    rekey = False
    if o.auto_rekey:
        if why:
            rekey = True
        else:
            if overlap < o.rekey_overlap:
                flags |= _capi.KF_LOW_OVERLAP
                rekey = True
            if o.max_age > 0 and age >= o.max_age:
                flags |= _capi.KF_MAX_AGE
                rekey = True
    if rekey:
        flags |= _capi.KF_REKEYED
        keyframes += 1
    ns = dict(has_key=1, age=0 if rekey else age, keyframes=keyframes, key_px=np.zeros(8, np.float32) if rekey else key, h_origin_key=hc if rekey else ho)
    return ns, dict(start_px=start, key_px=key, h_origin_curr=hc, overlap=overlap, age=age, keyframes=keyframes, flags=flags), int(rekey)


# ---- frame sequences

def render(cv, pose):
    """the frame of a camera whose pose is the offsets `pose` [8] against the canvas crop: frame(q) = scene(H(pose)^-1 q), as synth.make_pair renders img2"""
    pad = synth._PAD
    hinv = np.linalg.inv(homography(pose))
    vs, us = np.meshgrid(np.arange(synth.IMG_H, dtype=np.float64), np.arange(synth.IMG_W, dtype=np.float64), indexing="ij")
    xw = hinv[0, 0] * us + hinv[0, 1] * vs + hinv[0, 2]
    yw = hinv[1, 0] * us + hinv[1, 1] * vs + hinv[1, 2]
    zw = hinv[2, 0] * us + hinv[2, 1] * vs + hinv[2, 2]
    img = np.floor(synth._bilinear(cv, xw / zw + pad, yw / zw + pad) + 0.5)
    return np.clip(img, 0, 255).astype(np.uint8)


def relative(pose_a, pose_b):
    """the true offsets a -> b of two frames rendered at poses a and b: b(H p) = a(p) for H = H(pose_b) . H(pose_a)^-1"""
    return corners(homography(pose_b) @ np.linalg.inv(homography(pose_a)))


@functools.lru_cache(maxsize=None)
def sequence(name, seed):
    """-> (frames u8 [F, 224, 320], poses f64 [F, 8] against frame 0, noisy steps f32 [F, 8] (row i: frame i - 1 -> i, truth plus synth.make_prior's
    bounded noise of sigma 0.3 px; row 0 zero)).  Motions stay inside the canvas' 48 px border.
    out-and-back: 4 frames out along synth.true_offsets(seed, 5.0) per frame (20 px at the most) and 4 back: frame 8 is frame 0's pose.
    translation-32: 4 px per frame to the right for 10 frames; at rekey_overlap = 0.9 the overlap falls below at 32 px (frame 8: 287 x 223 of 71 680
    pixels).  Whole pixels: the frames are exact resamplings of one another, so the row's error is fp32 rounding and the row tests the re-key and the
    origin chain, not sub-pixel accuracy (out-and-back does)."""
    cv = synth.canvas(seed)
    if name == "out-and-back":
        d = synth.true_offsets(seed, 5.0)
        poses = [d * k for k in (0, 1, 2, 3, 4, 3, 2, 1, 0)]
    elif name == "translation-32":
        poses = [np.tile(np.array([4.0 * k, 0.0]), 4) for k in range(11)]
    else:
        raise KeyError(name)
    poses = np.stack(poses)
    frames = np.stack([render(cv, p) for p in poses])
    steps = np.zeros((len(poses), 8), np.float32)
    for i in range(1, len(poses)):
        steps[i] = synth.make_prior(seed * 100 + i, relative(poses[i - 1], poses[i]), STEP_SIGMA)
    return frames, poses, steps


def chained_sum(steps, upto):
    """the plain sum of the steps' offsets up to frame `upto`: what integrating frame-to-frame measurements gives"""
    return steps[1:upto + 1].astype(np.float64).sum(axis=0)


# ---- the host reference

def build_ref(tmp):
    so = str(tmp / "keyframe_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", *U.HOST_FLAGS, os.path.join(ROOT, "tests", "cpp", "keyframe_ref.cpp"), "-o", so],
                   check=True)
    return C.CDLL(so)


def ref_compose(lib, step, key):
    """-> offsets f32 [8], or None when the header's compose fails (nothing written)"""
    s, k = np.ascontiguousarray(step, np.float32).reshape(8), np.ascontiguousarray(key, np.float32).reshape(8)
    out = np.full(8, -777.0, np.float32)
    ok = lib.keyframe_ref_compose(C.c_void_p(s.ctypes.data), C.c_void_p(k.ctypes.data), C.c_void_p(out.ctypes.data))
    if not ok:
        assert (out == -777.0).all()
        return None
    return out


def new_state():
    return np.zeros(1, STATE)


def ref_decide(lib, state, start, rec, o, gap=False):
    """-> (new state [1] STATE, output record [1] TRACK, copy) of the header's decide"""
    st = np.ascontiguousarray(state, STATE).reshape(1)
    s = np.ascontiguousarray(start, np.float32).reshape(8)
    r = np.ascontiguousarray(rec, REC).reshape(1)
    ns, out = np.zeros(1, STATE), np.zeros(1, TRACK)
    out.view(np.uint8)[:] = 0xA5                                         # every byte must be written
    copy = lib.keyframe_ref_decide(C.c_void_p(st.ctypes.data), C.c_void_p(s.ctypes.data), C.c_void_p(r.ctypes.data), C.byref(o), int(gap), C.c_void_p(ns.ctypes.data),
                                   C.c_void_p(out.ctypes.data))
    return ns, out, int(copy)


class RefSession:
    """one session on the host reference: its state and its keyframe"""

    def __init__(self, lib):
        self.lib, self.state, self.key = lib, new_state(), np.zeros((224, 320), np.uint8)

    def track(self, curr, step, o, gap=False):
        c = np.ascontiguousarray(curr, np.uint8).reshape(224, 320)
        s = None if step is None else np.ascontiguousarray(step, np.float32).reshape(8)
        out = np.zeros(1, TRACK)
        self.lib.keyframe_ref_track(C.c_void_p(self.state.ctypes.data), C.c_void_p(self.key.ctypes.data), C.c_void_p(c.ctypes.data),
                                    C.c_void_p(s.ctypes.data) if s is not None else None, C.byref(o), int(gap), C.c_void_p(out.ctypes.data))
        return out[0]

    def reset(self):
        self.state[:] = 0


@functools.lru_cache(maxsize=None)
def _ref_rows_cached(lib_path, name, seed):
    lib = C.CDLL(lib_path)
    frames, _, steps = sequence(name, seed)
    ses, o = RefSession(lib), opts(rekey_overlap=ROWS[name][0])
    return np.stack([ses.track(frames[i], steps[i], o) for i in range(len(frames))])


def ref_row(lib, name, seed):
    """the host reference's records [F] of a row's sequence (computed once per library and shared)"""
    return _ref_rows_cached(lib._name, name, seed)


def truth_key_px(poses, recs):
    """the true key -> curr offsets [F, 8] given the records' re-keys (frame 0 is the first keyframe)"""
    out, key = np.zeros((len(poses), 8)), 0
    for i in range(len(poses)):
        out[i] = relative(poses[key], poses[i])
        if recs[i]["flags"] & _capi.KF_REKEYED:
            key = i
    return out


def worst_key_px(recs, poses):
    return float(np.abs(recs["key_px"].astype(np.float64) - truth_key_px(poses, recs)).max())


def worst_origin_px(recs, poses):
    """worst-component distance (px) of the corners of h_origin_curr from the true pose, over all frames"""
    return float(max(np.abs(corners(r["h_origin_curr"]) - p).max() for r, p in zip(recs, poses)))
