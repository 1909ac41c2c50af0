"""What the CPU and the GPU tests of recovering a lost camera inside the in-step keyframe track share (include/hnet.h hnet_filters_set_keyframe_recover;
DESIGN 7y): the host reference tests/cpp/filters_keyframe_recover_ref.cpp behind ctypes, the record layout, one filter session on the host (a
keyframe_recover_util.RefRecoverSession and its prev_ok word) and the four rows of keyframe_recover_util.ROWS with their steps loaded into the filter's
offset states."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import filters_keyframe_util as FK
import keyframe_recover_util as KR
import keyframe_util as K
import photo_align_util as U
import photo_search_oriented_util as O
from cuahn_vio_amd import _capi

ROOT = U.ROOT
RECORD = _capi.KEYFRAME_MEASURE_RECOVER_DTYPE
FROM_RELOC, REATTACHED = 65536, 131072
UNUSABLE = FK.UNUSABLE | REATTACHED
SEEDS = KR.SEEDS
assert RECORD.itemsize == 2448 + 2040 and RECORD.fields["reloc"][1] == 2448

# z_px of the frame AFTER a recovery (frame 2 of the rows without a map, frame 6 of the map rows) against keyframe_util.relative of the true poses: the
# worst corner component [px] on the host reference, per row and seed (1, 2, 5, 11).  The gate of a row is twice its worst seed;
# tests/test_gpu_filters_keyframe_recover.py reproduces the figures to the printed digit.  Through today's code the same frames carry no measurement at
# all: the lost frame is TRACK_LOST and the frame after it PREV_NOT_MEASURED.  (DESIGN 7y holds the table.)
NEXT_Z = {"kidnapped": (0.2709, 0.4864, 0.1509, 0.0787), "turned": (0.0581, 0.0412, 0.0270, 0.0557),
          "kidnapped_map": (0.1689, 0.1791, 0.1264, 0.4312), "turned_map": (0.0080, 0.0094, 0.0172, 0.0085)}


def next_z_gate(name):
    return 2 * max(NEXT_Z[name])


def build_ref(tmp):
    so = str(tmp / "filters_keyframe_recover_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread", *U.HOST_FLAGS,
                    os.path.join(ROOT, "tests", "cpp", "filters_keyframe_recover_ref.cpp"), "-o", so], check=True)
    return build_cached(so)


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def ref_measure(lib, had_key, key_prev, prev_ok, track, accepted, reloc, accepted_reloc, o, k=10.0):
    """measure_recover -> (ok, z_px, r_px, out72, flags); the outputs are pre-filled with 7 so that 'nothing written' shows"""
    t = np.ascontiguousarray(track, FK.TRACK).reshape(1)
    r = np.ascontiguousarray(reloc, O.ORELOC).reshape(1)
    kp = np.ascontiguousarray(key_prev, np.float32).reshape(8)
    z, r_px, out72, flags = np.full(8, 7.0, np.float32), np.full((8, 8), 7.0), np.full(72, 7.0, np.float32), C.c_int32(0)
    ok = lib.filters_keyframe_recover_ref_measure(int(had_key), _p(kp), int(prev_ok), _p(t), int(accepted), _p(r), int(accepted_reloc), C.byref(o), C.c_double(k), _p(z),
                                                  _p(r_px), _p(out72), C.byref(flags))
    return ok, z, r_px, out72, flags.value


def plain_measure(lib, had_key, key_prev, prev_ok, track, accepted, o, k=10.0):
    """hnet_kfm::measure in the same build, same conventions"""
    t = np.ascontiguousarray(track, FK.TRACK).reshape(1)
    kp = np.ascontiguousarray(key_prev, np.float32).reshape(8)
    z, r_px, out72, flags = np.full(8, 7.0, np.float32), np.full((8, 8), 7.0), np.full(72, 7.0, np.float32), C.c_int32(0)
    ok = lib.filters_keyframe_recover_ref_plain_measure(int(had_key), _p(kp), int(prev_ok), _p(t), int(accepted), C.byref(o), C.c_double(k), _p(z), _p(r_px), _p(out72),
                                                        C.byref(flags))
    return ok, z, r_px, out72, flags.value


def ref_relative_z(lib, key_prev, key_curr):
    a, b = np.ascontiguousarray(key_prev, np.float32).reshape(8), np.ascontiguousarray(key_curr, np.float32).reshape(8)
    z = np.full(8, -777.0, np.float32)
    return z if lib.filters_keyframe_recover_ref_relative_z(_p(a), _p(b), _p(z)) else None


def ref_innovation(lib, st, p, z_px, r_px):
    """hnet_ekf::innovation of {z_px | (float)(r_px / k_net_cov)} on the state -> the record (iteration 0)"""
    s = np.ascontiguousarray(st, FK.FSTATE).reshape(1)
    inn = np.zeros(1, FK.INNOV)
    lib.filters_keyframe_recover_ref_innovation(_p(s), C.byref(p), _p(np.ascontiguousarray(z_px, np.float32)), _p(np.ascontiguousarray(r_px, np.float64)), _p(inn))
    return inn[0]


class RefFilterSession:
    """one measuring session on the host: a keyframe_recover_util.RefRecoverSession (state, keyframe, map) and the prev_ok word"""

    def __init__(self, lib, capacity):
        self.lib, self.ses, self.prev_ok = lib, KR.RefRecoverSession(lib, capacity), 0

    def clone(self):
        other = RefFilterSession.__new__(RefFilterSession)
        other.lib, other.ses, other.prev_ok = self.lib, self.ses.clone(), self.prev_ok
        return other

    def snapshot(self):
        return self.ses.snapshot() + (self.prev_ok,)

    def step(self, st, p, net, gate, max_nis, measure, reloc, hyps, curr, gap=False, measured=False, align_rec=None, accepted=0, script=None, max_ratio=0.0):
        """hnet_ekf::iterated_update_keyframe_recovered (measured: iterated_update_keyframe_measured) on a copy of the state; the session advances ->
        dict(state, updates, innov, prec, rec [RECORD], counts)"""
        s = np.ascontiguousarray(st, FK.FSTATE).reshape(1).copy()
        iters = len(net)
        nn = np.ascontiguousarray(net, dtype=np.float32)
        sc = np.zeros(1 + iters, FK.PHOTO) if script is None else np.ascontiguousarray(script, FK.PHOTO)
        ses = np.zeros(1, FK.SESSION)
        ses["key"], ses["prev_ok"] = self.ses.state[0], self.prev_ok
        cur = np.ascontiguousarray(curr, np.uint8).reshape(224, 320)
        ar = None if align_rec is None else np.ascontiguousarray(align_rec, _capi.PHOTO_ROBUST_DTYPE).reshape(1)
        h = None if hyps is None else np.ascontiguousarray(hyps, O.HYP)
        rec, prec, rout, counts = np.zeros(iters, FK.INNOV), np.zeros(1 + iters, FK.PHOTO), np.zeros(1, RECORD), np.zeros(3, np.int32)
        a = self.ses
        u = self.lib.filters_keyframe_recover_ref_iterated(
            int(measured), _p(s), C.byref(p), iters, _p(nn), int(gate), C.c_double(max_nis), _p(sc), C.c_double(max_ratio), 0,
            C.byref(measure) if measure is not None else None, C.byref(reloc) if reloc is not None else None, _p(h), 0 if h is None else len(h), int(gap), _p(ses),
            _p(a.key), _p(a.mstate), _p(a.entries), _p(a.images), int(a.capacity), _p(cur), _p(ar), int(accepted), _p(rec), _p(prec), _p(rout), _p(counts))
        a.state[0] = ses["key"][0]
        self.prev_ok = int(ses["prev_ok"][0])
        return dict(state=s, updates=u, innov=rec, prec=prec, rec=rout[0], counts=counts)


# ---- the rows: keyframe_recover_util.ROWS with the rows' steps as the filter's offset states, a network that applies nothing, cov_scale = 1

def row_measure_opts(name):
    t = KR.track_opts(name)
    return _capi.KeyframeMeasureOpts(t, 1.0, 0.05, 0.0, FK.ALWAYS, 0)


def row_params():
    import test_filters_innov_cpu as ti
    return ti._params(1e12)


def row_net():
    net = np.zeros((1, 72), np.float32)
    net[0, 8:] = np.eye(8, dtype=np.float32).reshape(64)
    return net


def row_step(r, i):
    return np.zeros(8, np.float32) if r["steps"][i] is None else np.asarray(r["steps"][i], np.float32)


def row_time(i):
    return 1.0 + 0.1 * i


def run_row(lib, tab, name, seed, max_nis=0.0, recover=True, check=None):
    """the row through the host loop -> the per-frame dicts of RefFilterSession.step.  check(i, before, after, out): called after every frame with the
    session as it was and as it is"""
    r = KR.row(name, seed)
    fs = RefFilterSession(lib, KR.capacity(name))
    mo, ro, p, net = row_measure_opts(name), KR.reloc_opts(name), row_params(), row_net()
    outs = []
    for i, frame in enumerate(r["frames"]):
        before = fs.clone()
        st = FK.row_state(row_step(r, i), row_time(i))
        out = fs.step(st, p, net, 0, max_nis, mo, ro if recover else None, tab if recover else None, frame)
        if check is not None:
            check(i, before, fs, out)
        outs.append(out)
    return outs


@functools.lru_cache(maxsize=None)
def _row_cached(lib_path, name, seed, max_nis, recover):
    lib = build_cached(lib_path)
    return run_row(lib, O.yaw_table(lib), name, seed, max_nis, recover)


@functools.lru_cache(maxsize=None)
def build_cached(lib_path):
    lib = C.CDLL(lib_path)
    lib.photo_search_ref_better.argtypes = [C.c_double, C.c_int, C.c_double, C.c_int]
    lib.photo_search_oriented_ref_make_hyp.argtypes = [C.c_double, C.c_double, C.c_void_p]
    lib.photo_search_oriented_ref_yaw_table.argtypes = [C.c_double, C.c_double, C.c_int, C.c_void_p]
    return lib


def ref_row(lib, name, seed, max_nis=0.0, recover=True):
    """run_row, computed once per (row, seed, gate, recover) and shared; do not modify what it returns"""
    return _row_cached(lib._name, name, seed, float(max_nis), bool(recover))


def next_z_error(name, seed, z_px):
    """the worst corner component [px] of the z_px of the frame after the recovery against the true relative pose"""
    r = KR.row(name, seed)
    return float(np.abs(np.asarray(z_px, np.float64) - K.relative(r["pose"], r["next_pose"])).max())
