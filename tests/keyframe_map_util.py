"""What the CPU and the GPU tests of the keyframe map share (include/hnet.h hnet_sessions_enable_keyframe_map, hnet_sessions_keyframe_revisit):
the three accuracy rows and their gates, the host reference tests/cpp/keyframe_map_ref.cpp behind ctypes, a numpy float64 restatement of relative, the
grid count and select, and the record layouts.  Sequences, options of the track and the geometry helpers are keyframe_util's."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import keyframe_util as K
import photo_align_util as U
from cuahn_vio_amd import _capi

ENTRY, MSTATE, REVISIT = _capi.KEYFRAME_MAP_ENTRY_DTYPE, _capi.KEYFRAME_MAP_STATE_DTYPE, _capi.KEYFRAME_REVISIT_DTYPE
assert ENTRY.itemsize == 88 and MSTATE.itemsize == 16 and REVISIT.itemsize == 1864
CAPACITY = 3                               # the capacity of every test unless stated
TRACK_OPTS = dict(max_age=1)               # every row re-keys at every frame: the chain gets one link per frame

# The accuracy rows: name -> (frame replaced by a constant 128 image or None, frame the revisit follows, the two frames tracked after it, gate in px).
# All on keyframe_util.sequence("out-and-back", seed), seeds 1, 2, 5, 11, tracked with max_age = 1.  A gate is TWICE the worst distance (worst corner
# component, px) of the host reference's h_origin_curr AFTER the revisit from the true pose over the seeds, as
# tests/test_keyframe_map_cpu.py::test_accuracy_rows prints it (DESIGN 7q holds the measured values)
ROWS = {
    "closure-at-origin": (None, 8, (1, 2), 2 * 2.662e-5),
    "closure-sub-pixel": (None, 6, (7, 8), 2 * 0.03384),
    "recovery": (4, 5, (6, 7), 2 * 0.04946),
}
BEFORE_RATIO = 3.0                         # closure-at-origin and recovery: the chain before the revisit is at least this many gates off


def opts(levels=K.LEVELS, min_grid=32, min_overlap=0.5, max_mse=0.0, max_closure_px=0.0, **align):
    """hnet_keyframe_revisit_opts with the defaults of hnet_keyframe_revisit_default_opts and 6 trials (no library needed)"""
    a = dict(max_iterations=K.TRIALS)
    a.update(align)
    import photo_robust_util as R
    return _capi.KeyframeRevisitOpts(R.opts(**a), levels, min_grid, min_overlap, max_mse, max_closure_px)


def opts_kw(o):
    """the keyword form of `o` for HnetSessions.keyframe_revisit"""
    return dict(max_iterations=o.align.base.max_iterations, min_valid=o.align.base.min_valid, lambda0=o.align.base.lambda0, eps_px=o.align.base.eps_px,
                brightness=o.align.brightness, huber_k=o.align.huber_k, gain0=o.align.gain0, bias0=o.align.bias0, levels=o.levels, min_grid=o.min_grid,
                min_overlap=o.min_overlap, max_mse=o.max_mse, max_closure_px=o.max_closure_px)


# ---- the rule in float64 (numpy): the restatement the header is tested against

GRID = np.array([[20.0 + 40.0 * (i & 7), 14.0 + 28.0 * (i >> 3), 1.0] for i in range(64)])


FRAME_UNITS = np.array([[1.0, 1.0, 1 / 320.0], [1.0, 1.0, 1 / 320.0], [320.0, 320.0, 1.0]])    # a matrix conjugated by diag(1 / 320, 1 / 320, 1), entry by entry


def np_invertible(h):
    """the header's test of inverse: finite, and |det| at least 1e-12 times the cube of the largest entry in frame units"""
    h = np.asarray(h, np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        det = np.linalg.det(h) if np.isfinite(h).all() else np.nan
        return bool(np.isfinite(det) and det != 0.0 and abs(det) >= 1e-12 * np.abs(h * FRAME_UNITS).max() ** 3)


def np_relative(h_curr, h_key):
    """-> (G [3, 3] with G[2, 2] = 1, start [8] f64 unrounded) or None: G = h_curr . inverse(h_key) by LAPACK"""
    h_curr, h_key = np.asarray(h_curr, np.float64).reshape(3, 3), np.asarray(h_key, np.float64).reshape(3, 3)
    if not np.isfinite(h_curr).all() or not np_invertible(h_key):
        return None
    g = h_curr @ np.linalg.inv(h_key)
    if not np.isfinite(g).all() or abs(g[2, 2]) < 1e-12 * np.abs(g).max():
        return None
    g = g / g[2, 2]
    q = np.concatenate([K.P4.reshape(4, 2), np.ones((4, 1))], axis=1) @ g.T
    if not (q[:, 2] > 0).all():
        return None
    return g, K.corners(g)


def np_grid_count(g):
    q = GRID @ np.asarray(g, np.float64).reshape(3, 3).T
    with np.errstate(all="ignore"):
        x, y = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        return int(((q[:, 2] > 0) & (x >= 0) & (x <= 319) & (y >= 0) & (y <= 223)).sum())


def np_select(mstate, entries, h_curr, min_grid):
    """-> (slot or -1, grid, start [8] f64 or None): fewest links, then the larger grid count, then the lower slot"""
    best = None
    for slot, e in enumerate(entries):
        if not e["valid"] or slot == mstate["cur_slot"] or e["links"] >= mstate["cur_links"]:
            continue
        r = np_relative(h_curr, e["h_origin_key"])
        if r is None:
            continue
        grid = np_grid_count(r[0])
        if grid < min_grid:
            continue
        key = (int(e["links"]), -grid, slot)
        if best is None or key < best[0]:
            best = (key, slot, grid, r[1])
    return (-1, 0, None) if best is None else best[1:]


# ---- the host reference

def build_ref(tmp):
    so = str(tmp / "keyframe_map_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", *U.HOST_FLAGS, os.path.join(K.ROOT, "tests", "cpp", "keyframe_map_ref.cpp"),
                    "-o", so], check=True)
    return C.CDLL(so)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def new_map(capacity=CAPACITY):
    """-> (entries [capacity], map state [1]) of an empty map"""
    return np.zeros(capacity, ENTRY), np.zeros(1, MSTATE)


def ref_note(lib, flags, copy, new_state, mstate, entries):
    """the header's note -> (store slot, new map state, new entries); the inputs are not modified"""
    m, e = np.ascontiguousarray(mstate, MSTATE).reshape(1).copy(), np.ascontiguousarray(entries, ENTRY).copy()
    ns = np.ascontiguousarray(new_state, K.STATE).reshape(1)
    slot = lib.keyframe_map_ref_note(int(flags), int(copy), _p(ns), _p(m), _p(e), len(e))
    return int(slot), m, e


def ref_origin_curr(lib, state):
    s, h = np.ascontiguousarray(state, K.STATE).reshape(1), np.zeros((3, 3))
    ok = lib.keyframe_map_ref_origin_curr(_p(s), _p(h))
    return bool(ok), h


def ref_relative(lib, h_curr, entry):
    """-> (G [3, 3], start f32 [8]) or None"""
    h, e = np.ascontiguousarray(h_curr, np.float64).reshape(3, 3), np.ascontiguousarray(entry, ENTRY).reshape(1)
    g, start = np.zeros((3, 3)), np.zeros(8, np.float32)
    return (g, start) if lib.keyframe_map_ref_relative(_p(h), _p(e), _p(g), _p(start)) else None


def ref_grid_count(lib, g):
    g = np.ascontiguousarray(g, np.float64).reshape(3, 3)
    return int(lib.keyframe_map_ref_grid_count(_p(g)))


def ref_select(lib, mstate, entries, h_curr, min_grid):
    """-> (slot or -1, grid, start f32 [8]) of the header's select"""
    m, e = np.ascontiguousarray(mstate, MSTATE).reshape(1), np.ascontiguousarray(entries, ENTRY)
    h, start, grid = np.ascontiguousarray(h_curr, np.float64).reshape(3, 3), np.zeros(8, np.float32), C.c_int(0)
    slot = lib.keyframe_map_ref_select(_p(m), _p(e), len(e), _p(h), int(min_grid), _p(start), C.byref(grid))
    return int(slot), int(grid.value), start


def ref_decide(lib, state, mstate, entries, cand, grid, start, h_before, rec, o):
    """-> (new state [1], new map state [1], output record [1] REVISIT, attach) of the header's decide_revisit"""
    s, m, e = np.ascontiguousarray(state, K.STATE).reshape(1), np.ascontiguousarray(mstate, MSTATE).reshape(1), np.ascontiguousarray(entries, ENTRY)
    st, hb = np.ascontiguousarray(start, np.float32).reshape(8), np.ascontiguousarray(h_before, np.float64).reshape(3, 3)
    r = np.ascontiguousarray(rec, K.REC).reshape(1)
    ns, nm, out = np.zeros(1, K.STATE), np.zeros(1, MSTATE), np.zeros(1, REVISIT)
    out.view(np.uint8)[:] = 0xA5                                         # every byte must be written
    attach = lib.keyframe_map_ref_decide(_p(s), _p(m), _p(e), int(cand), int(grid), _p(st), _p(hb), _p(r), C.byref(o), _p(ns), _p(nm), _p(out))
    return ns, nm, out, int(attach)


class RefMapSession:
    """one session on the host reference: its state, its keyframe, and its map's entries, state and images"""

    def __init__(self, lib, capacity=CAPACITY):
        self.lib, self.state, self.key = lib, K.new_state(), np.zeros((224, 320), np.uint8)
        self.entries, self.mstate = new_map(capacity)
        self.images = np.zeros((capacity, 224, 320), np.uint8)

    def track(self, curr, step, o, gap=False):
        c = np.ascontiguousarray(curr, np.uint8).reshape(224, 320)
        s = None if step is None else np.ascontiguousarray(step, np.float32).reshape(8)
        out = np.zeros(1, K.TRACK)
        self.lib.keyframe_map_ref_track(_p(self.state), _p(self.key), _p(self.mstate), _p(self.entries), _p(self.images), len(self.entries), _p(c),
                                        _p(s) if s is not None else None, C.byref(o), int(gap), _p(out))
        return out[0]

    def revisit(self, curr, o):
        c = np.ascontiguousarray(curr, np.uint8).reshape(224, 320)
        out = np.zeros(1, REVISIT)
        self.lib.keyframe_map_ref_revisit(_p(self.state), _p(self.key), _p(self.mstate), _p(self.entries), _p(self.images), len(self.entries), _p(c), C.byref(o),
                                          _p(out))
        return out[0]

    def reset(self):
        self.state[:] = 0
        self.entries[:] = 0
        self.mstate[:] = 0


# ---- the rows

def row_frames(name, seed):
    """-> (frames [9] with the row's lost frame replaced, poses, steps) of the row"""
    lost, _, _, _ = ROWS[name]
    frames, poses, steps = K.sequence("out-and-back", seed)
    if lost is not None:
        frames = frames.copy()
        frames[lost] = 128
    return frames, poses, steps


def run_row(name, seed, track, revisit, before_revisit=None):
    """the row on any session: track(frame, step) -> TRACK record for frames 0 .. the revisit's, before_revisit() if given, revisit(frame) -> REVISIT
    record, then the two tracks after it -> (track records up to the revisit, the revisit's record, the two track records after it)"""
    _, at, after, _ = ROWS[name]
    frames, _, steps = row_frames(name, seed)
    recs = [track(frames[i], steps[i]) for i in range(at + 1)]
    if before_revisit is not None:
        before_revisit()
    rv = revisit(frames[at])
    return np.stack(recs), rv, np.stack([track(frames[i], steps[i]) for i in after])


@functools.lru_cache(maxsize=None)
def _ref_row_cached(lib_path, name, seed, capacity):
    ses = RefMapSession(C.CDLL(lib_path), capacity)
    to, ro = K.opts(**TRACK_OPTS), opts()
    recs, rv, after = run_row(name, seed, lambda f, s: ses.track(f, s, to), lambda f: ses.revisit(f, ro))
    return recs, rv, after, ses


def ref_row(lib, name, seed, capacity=CAPACITY):
    """the host reference's run of a row (computed once per library and shared; nobody modifies it): (track records, revisit record, the two track
    records after it, the session as the row left it)"""
    return _ref_row_cached(lib._name, name, seed, capacity)


def worst_px(h, pose):
    """worst-component distance (px) of the corners of h from the true pose"""
    return float(np.abs(K.corners(h) - pose).max())
