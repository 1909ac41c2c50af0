"""What the CPU and the GPU tests of recovering a lost camera inside the track share (include/hnet.h hnet_sessions_keyframe_track_recover):
the host reference tests/cpp/keyframe_recover_ref.cpp behind ctypes, one session's whole call on it, the two twins built from the existing reference calls
alone, the four rows (photo_search_util's and photo_search_oriented_util's kidnapped rows under auto_rekey = 1 and max_mse = 120) and the record layouts.
Frames, gates and the older references are the older utilities'."""
import copy
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import keyframe_map_util as KM
import keyframe_util as K
import photo_align_util as U
import photo_search_oriented_util as O
import photo_search_util as S
from cuahn_vio_amd import _capi, synth

ROOT = U.ROOT
RECOVER = _capi.KEYFRAME_RECOVER_DTYPE
STASH = np.dtype([("state", K.STATE), ("start_px", "<f4", 8), ("key_px", "<f4", 8), ("h_origin_curr", "<f8", (3, 3)), ("overlap", "<f8"), ("age", "<i4"),
                  ("keyframes", "<i4"), ("flags", "<i4"), ("copy", "<i4")])
assert RECOVER.itemsize == 1720 + 2040 and STASH.itemsize == 280
SEEDS = S.SEEDS
NOT_LOST, RECOVERED, UNRECOVERED = 0, 1, 2          # what RefRecoverSession.track_recover returns besides the record

# The rows' track options: auto_rekey = 1 (the default) and max_mse = 120.  Honest tracks of these rows have mse of at most 36.81 and the kidnapped or
# constant frames at least 395.7 on the host reference (seeds 1, 2, 5, 11): 120 separates them by more than 3 on either side, which
# tests/test_keyframe_recover_cpu.py::test_rows asserts on every frame.
MAX_MSE = 120.0
HONEST_BELOW, LOST_ABOVE = MAX_MSE / 3.0, MAX_MSE * 3.0
ROWS = ("kidnapped", "turned", "kidnapped_map", "turned_map")


def track_opts(row, auto_rekey=1):
    if row.endswith("_map"):
        return K.opts(levels=K.LEVELS, auto_rekey=auto_rekey, max_mse=MAX_MSE, **KM.TRACK_OPTS)
    return K.opts(levels=S.LEVELS, auto_rekey=auto_rekey, max_mse=MAX_MSE)


def reloc_opts(row):
    return S.reloc_opts(min_overlap=O.TURNED_MIN_OVERLAP) if row == "turned" else S.reloc_opts()


def recover_opts(track, reloc):
    """hnet_keyframe_recover_opts of the two blocks (no library needed)"""
    return _capi.KeyframeRecoverOpts(track, reloc)


def gate(row):
    return {"kidnapped": S.GATE_KIDNAPPED, "turned": O.GATE_TURNED, "kidnapped_map": S.GATE_KIDNAPPED_MAP, "turned_map": O.GATE_TURNED_MAP}[row]


def capacity(row):
    return S.CAPACITY if row.endswith("_map") else 0


# ---- the host reference

def build_ref(tmp):
    so = str(tmp / "keyframe_recover_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", *U.HOST_FLAGS, os.path.join(ROOT, "tests", "cpp", "keyframe_recover_ref.cpp"),
                    "-o", so], check=True)
    lib = C.CDLL(so)
    lib.photo_search_ref_better.argtypes = [C.c_double, C.c_int, C.c_double, C.c_int]
    lib.photo_search_oriented_ref_make_hyp.argtypes = [C.c_double, C.c_double, C.c_void_p]
    lib.photo_search_oriented_ref_yaw_table.argtypes = [C.c_double, C.c_double, C.c_int, C.c_void_p]
    return lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def ref_decide(lib, state, start, rec, o, gap=False):
    """-> (new state [1], track record [1], stash [1], active, copy) of the header's decide_deferred"""
    st = np.ascontiguousarray(state, K.STATE).reshape(1)
    s = np.ascontiguousarray(start, np.float32).reshape(8)
    r = np.ascontiguousarray(rec, K.REC).reshape(1)
    ns, out, stash, active = np.zeros(1, K.STATE), np.zeros(1, K.TRACK), np.zeros(1, STASH), C.c_int(-1)
    out.view(np.uint8)[:] = 0xA5                                         # every byte must be written
    stash.view(np.uint8)[:] = 0xA5
    cp = lib.keyframe_recover_ref_decide(_p(st), _p(s), _p(r), C.byref(o), int(gap), _p(ns), _p(out), _p(stash), C.byref(active))
    return ns, out, stash, int(active.value), int(cp)


def ref_finish(lib, reloc_flags, stash, state, track):
    """-> (state [1], track record [1], copy2) of the header's finish; the inputs are not modified"""
    s, t = np.ascontiguousarray(state, K.STATE).reshape(1).copy(), np.ascontiguousarray(track, K.TRACK).reshape(1).copy()
    st = np.ascontiguousarray(stash, STASH).reshape(1)
    return s, t, int(lib.keyframe_recover_ref_finish(int(reloc_flags), _p(st), _p(s), _p(t)))


def zero_reloc(lib):
    out = np.zeros(1, O.ORELOC)
    out.view(np.uint8)[:] = 0xA5
    lib.keyframe_recover_ref_zero_reloc(_p(out))
    return out[0]


class RefRecoverSession(O.RefSession):
    """photo_search_oriented_util.RefSession with the track that recovers; capacity 0: no map"""

    def track_recover(self, curr, step, o, hyps, gap=False, given_track=None, given_reloc=None):
        """o: a KeyframeRecoverOpts; given_*: level-0 alignment records to decide on instead of the host alignment's -> (RECOVER record, outcome)"""
        c = np.ascontiguousarray(curr, np.uint8).reshape(224, 320)
        s = None if step is None else np.ascontiguousarray(step, np.float32).reshape(8)
        gt = None if given_track is None else np.ascontiguousarray(given_track, K.REC).reshape(1)
        gr = None if given_reloc is None else np.ascontiguousarray(given_reloc, K.REC).reshape(1)
        h = np.ascontiguousarray(hyps, O.HYP)
        out = np.zeros(1, RECOVER)
        out.view(np.uint8)[:] = 0xA5
        what = self.lib.keyframe_recover_ref_track(_p(self.state), _p(self.key), _p(self.mstate), _p(self.entries), _p(self.images), int(self.capacity), _p(c),
                                                   _p(s) if s is not None else None, C.byref(o), _p(h), len(h), int(gap), _p(gt) if gt is not None else None,
                                                   _p(gr) if gr is not None else None, _p(out))
        return out[0], int(what)

    def clone(self):
        other = copy.copy(self)
        for name in ("state", "key", "mstate", "entries", "images"):
            setattr(other, name, getattr(self, name).copy())
        return other


def twins(before, curr, step, o, hyps, gap=False, lost=True):
    """the two twins of a call on clones of `before` (the session as it was), from the existing reference calls alone -> ((twin A, its track record),
    (twin B, its track record under auto_rekey = 0, its relocalise record)); twin B is None for a call that was not lost (nothing compares against it)"""
    a = before.clone()
    ta = a.track(curr, step, o.track, gap)
    if not lost:
        assert not ta["flags"] & _capi.KF_LOST
        return (a, ta), None
    b = before.clone()
    t0 = _capi.KeyframeOpts.from_buffer_copy(o.track)
    t0.auto_rekey = 0
    tb = b.track(curr, step, t0, gap)
    rb = b.relocalise_oriented(curr, o.reloc, hyps)
    return (a, ta), (b, tb, rb)


def check_against_twins(ses_after, out, what, twin_a, twin_b):
    """the identities: a call that is not lost or is unrecovered equals twin A; a recovered one equals twin B apart from the RECOVERED bit"""
    a, ta = twin_a
    b, tb, rb = twin_b if twin_b is not None else (None, None, None)
    assert (what == NOT_LOST) == (twin_b is None)
    if what == RECOVERED:
        want = tb.copy()
        assert want["flags"] & _capi.KF_LOST and not want["flags"] & _capi.KF_RECOVERED
        want["flags"] |= _capi.KF_RECOVERED
        assert out["track"].tobytes() == want.tobytes() and out["reloc"].tobytes() == rb.tobytes()
        assert ses_after.snapshot() == b.snapshot()
    else:
        assert out["track"].tobytes() == ta.tobytes(), (out["track"]["flags"], ta["flags"])
        assert ses_after.snapshot() == a.snapshot()
        if what == NOT_LOST:
            assert out["reloc"].tobytes() == zero_reloc(ses_after.lib).tobytes()
        else:
            assert out["reloc"].tobytes() == rb.tobytes() and rb["rv"]["flags"] & (_capi.RL_NO_CANDIDATE | _capi.RL_REJECTED)


# ---- the rows: -> (frames, steps (None: a zero step), the truth each checked frame is measured against, the indices of the lost frames)

@functools.lru_cache(maxsize=None)
def row(name, seed):
    """-> dict(frames [F], steps (list of [8] f32 or None), lost: the index of the kidnapped frame, pose: its true pose [8], constant: the index of the
    constant frame or None, next: the index of the frame tracked after the kidnapped one with the true step)"""
    if name in ("kidnapped", "turned"):
        frames, poses, step = S.kidnapped(seed) if name == "kidnapped" else O.turned(seed)
        return dict(frames=frames, steps=[None, None, step], lost=1, pose=poses[1], constant=None, next=2, next_pose=poses[2])
    frames, steps, pose = S.kidnapped_map(seed) if name == "kidnapped_map" else O.turned_map(seed)
    pose2 = pose + synth.true_offsets(seed + 400, 2.0)
    frames = np.concatenate([frames, K.render(synth.canvas(seed), pose2)[None]])
    return dict(frames=frames, steps=[steps[i] for i in range(5)] + [None, K.relative(pose, pose2).astype(np.float32)], lost=5, pose=pose, constant=4, next=6,
                next_pose=pose2)


def row_error(name, rec, pose):
    """the row's error after the call (worst corner component, px): key_px of the relocalise in the rows without a map, its h_origin_curr with one"""
    if name.endswith("_map"):
        return KM.worst_px(rec["reloc"]["rv"]["h_origin_curr"], pose)
    return S.worst_px(rec["reloc"]["rv"]["key_px"], pose)


def plain_error(name, rec, pose):
    """the same frame through the plain track: its key_px (the bridge) without a map, its h_origin_curr with one"""
    if name.endswith("_map"):
        return KM.worst_px(rec["h_origin_curr"], pose)
    return S.worst_px(rec["key_px"], pose)
