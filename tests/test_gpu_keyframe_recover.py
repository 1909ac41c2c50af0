"""Recovering a lost camera inside the track on the device (include/hnet.h hnet_sessions_keyframe_track_recover; csrc/kernels_keyframe_recover.hip;
DESIGN 7u): a call in which nobody is lost against a twin fleet's keyframe_track; the four kidnapped rows against the host headers, against twin fleets
built from keyframe_track and keyframe_relocalise_oriented alone and against the operators; four different outcomes in one call; a NaN step; read-only for
everything the sessions had before; and the refusals.  Sessions objects of 4 cameras on a context of max_batch 8, capacity 0 and 3.  Every comparison is
byte for byte.

As in tests/test_gpu_keyframe_reloc_oriented.py "the host headers" are the shared headers run on the host (tests/cpp/keyframe_recover_ref.cpp) on the
alignment records of the device: the search is integers and the decisions are the same functions, while the host's own alignment sums in another order."""
import ctypes as C

import numpy as np
import pytest

import keyframe_recover_util as KR
import keyframe_util as K
import photo_search_oriented_util as O
import photo_search_util as S
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, CAPACITY = 1, 4, 5
N_CAM = 4


@pytest.fixture(scope="module")
def oref(tmp_path_factory):
    return KR.build_ref(tmp_path_factory.mktemp("keyframe_recover_ref_gpu"))


@pytest.fixture(scope="module")
def tab(oref):
    return O.yaw_table(oref)


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=8)
    yield e
    e.close()


@pytest.fixture
def fleet(eng):
    from cuahn_vio_amd.homography_net import HnetSessions
    made = []

    def make(capacity=S.CAPACITY, keyframes=True):
        s = HnetSessions(eng, N_CAM)
        if keyframes:
            s.enable_keyframes()
            if capacity:
                s.enable_keyframe_map(capacity)
        made.append(s)
        return s
    yield make
    for s in made:
        s.close()


def store(s, cam, capacity):
    """every byte the keyframe layers hold of a session: the keyframe, and with a map the entries, the map state and the images"""
    if not s.image_count(cam):
        return ()
    try:
        out = [s.keyframe(cam).tobytes()]
    except Exception:
        return ()
    if capacity:
        entries, mstate = s.keyframe_map_info(cam)
        out += [entries.tobytes(), mstate.tobytes()] + [s.map_keyframe(cam, i).tobytes() for i in range(capacity)]
    return tuple(out)


def zero_reloc():
    z = np.zeros(1, O.ORELOC)
    z["target"] = _capi.RL_TARGET_NONE
    return z[0]


class Cam:
    """a camera of a device fleet, its mirror on the host headers and its twin on a second fleet that only knows the older calls"""

    def __init__(self, s, twin, cam, lib, capacity, tab, o):
        self.s, self.twin, self.cam, self.capacity, self.tab, self.o = s, twin, cam, capacity, tab, o
        self.mir = KR.RefRecoverSession(lib, capacity)
        self.t0 = _capi.KeyframeOpts.from_buffer_copy(o.track)
        self.t0.auto_rekey = 0

    def recover(self, eng, frame, step):
        """one call on the fleet, checked against the mirror, the twin and the operators -> (record, outcome)"""
        held = self.mir.key.copy()
        had_key = bool(self.mir.state["has_key"][0])
        images = self.mir.images.copy()
        st = None if step is None else step[None]
        self.s.push([self.cam], frame[None])
        out = self.s.keyframe_track_recover([self.cam], st, hyps=self.tab, track=self.o.track, reloc=self.o.reloc)[0]
        want, what = self.mir.track_recover(frame, step, self.o, self.tab, given_track=out["track"]["rec"], given_reloc=out["reloc"]["rv"]["rec"])
        assert out.tobytes() == want.tobytes(), (out["track"]["flags"], want["track"]["flags"], out["reloc"]["rv"]["flags"], want["reloc"]["rv"]["flags"])
        assert store(self.s, self.cam, self.capacity) == self._mirror_store()
        # the twin: the older calls alone
        self.twin.push([self.cam], frame[None])
        if what == KR.RECOVERED:
            tt = self.twin.keyframe_track([self.cam], st, **K.opts_kw(self.t0))[0].copy()
            rr = self.twin.keyframe_relocalise_oriented([self.cam], hyps=self.tab, **S.reloc_kw(self.o.reloc))[0]
            tt["flags"] |= _capi.KF_RECOVERED
            assert out["track"].tobytes() == tt.tobytes() and out["reloc"].tobytes() == rr.tobytes()
        else:
            tt = self.twin.keyframe_track([self.cam], st, **K.opts_kw(self.o.track))[0]
            assert out["track"].tobytes() == tt.tobytes()
            if what == KR.NOT_LOST:
                assert out["reloc"].tobytes() == zero_reloc().tobytes()
        assert store(self.s, self.cam, self.capacity) == store(self.twin, self.cam, self.capacity)
        # the operators
        if had_key:
            rec = eng.op_photo_align_robust(held[None], frame[None], out["track"]["start_px"][None], levels=self.o.track.levels, max_iterations=S.TRIALS)
            assert out["track"]["rec"].tobytes() == rec[0].tobytes()
        if what != KR.NOT_LOST and out["reloc"]["target"] != _capi.RL_TARGET_NONE:
            candidate = held if out["reloc"]["target"] == _capi.RL_TARGET_HELD else images[int(out["reloc"]["target"])]
            r = out["reloc"]
            assert r["search"].tobytes() == eng.op_photo_search_oriented(candidate[None], frame[None], hyps=self.tab, **S.search_kw(self.o.reloc.search))[0].tobytes()
            start = r["search"]["base"]["start_px"]
            rec = eng.op_photo_align_robust(candidate[None], frame[None], start[None], levels=self.o.reloc.levels, max_iterations=S.TRIALS)
            assert r["rv"]["rec"].tobytes() == rec[0].tobytes() and r["rv"]["start_px"].tobytes() == start.tobytes()
        return out, what

    def _mirror_store(self):
        out = [self.mir.key.tobytes()]
        if self.capacity:
            out += [self.mir.entries.tobytes(), self.mir.mstate.tobytes()] + [self.mir.images[i].tobytes() for i in range(self.capacity)]
        return tuple(out)


def test_nobody_lost(fleet, tab):
    """three honest sessions listed out of order: the track records, the keyframes and the maps are a twin fleet's keyframe_track, the relocalise records
    are the zero record"""
    frames, _, steps = K.sequence("out-and-back", 5)
    a, b = fleet(), fleet()
    ids = [3, 0, 2]
    to = K.opts(max_mse=KR.MAX_MSE, max_age=2)
    seen = 0
    for i in range(4):
        f = np.stack([frames[i], frames[i + 1], frames[i + 2]])
        st = np.stack([steps[i], steps[i + 1], steps[i + 2]]) if i else None
        for s in (a, b):
            s.push(ids, f)
        out = a.keyframe_track_recover(ids, st, hyps=tab, track=to, reloc=S.reloc_opts())
        want = b.keyframe_track(ids, st, **K.opts_kw(to))
        assert out["track"].tobytes() == want.tobytes() and not (out["track"]["flags"] & (_capi.KF_LOST | _capi.KF_RECOVERED)).any()
        assert all(r.tobytes() == zero_reloc().tobytes() for r in out["reloc"])
        assert a.last_keyframe_device_ms() > 0.0
        seen |= int(np.bitwise_or.reduce(out["track"]["flags"]))
        for c in range(N_CAM):
            assert store(a, c, S.CAPACITY) == store(b, c, S.CAPACITY)
    assert seen & _capi.KF_FIRST and seen & _capi.KF_MAX_AGE           # first keyframes and re-keys went through the call's first commit


@pytest.mark.parametrize("seed", KR.SEEDS)
@pytest.mark.parametrize("name", KR.ROWS)
def test_rows(eng, fleet, oref, tab, name, seed):
    """a row with auto_rekey = 1, max_mse = 120 and the default yaw table: every record equals the host headers on the device's alignment records, the
    twin fleet's older calls (the next track included) and the operators; the kidnapped frame is RECOVERED inside the row's CPU-fixed gate, the constant
    frame of the map rows is lost and unrecovered, the next frame is TRACKED"""
    r, cap = KR.row(name, seed), KR.capacity(name)
    cam = Cam(fleet(cap), fleet(cap), 2, oref, cap, tab, KR.recover_opts(KR.track_opts(name), KR.reloc_opts(name)))
    recs, whats = zip(*[cam.recover(eng, f, r["steps"][i]) for i, f in enumerate(r["frames"])])
    lost, nxt = recs[r["lost"]], recs[r["next"]]
    err = KR.row_error(name, lost, r["pose"])
    print(f"{name}, seed {seed}, device: outcomes {whats}; lost flags {lost['track']['flags']}, relocalise flags {lost['reloc']['rv']['flags']}, target "
          f"{lost['reloc']['target']}, entry {lost['reloc']['search']['hyp']}; {err:.4f} px (gate {KR.gate(name):.4f}); {cam.s.last_keyframe_device_ms():.3f} ms on device")
    assert whats[r["lost"]] == KR.RECOVERED and lost["track"]["flags"] & _capi.KF_RECOVERED and err <= KR.gate(name)
    if r["constant"] is None:
        assert lost["track"]["flags"] == _capi.KF_MSE_ABOVE_MAX | _capi.KF_BRIDGED | _capi.KF_RECOVERED and lost["reloc"]["rv"]["flags"] == _capi.RL_RETRACKED
        assert float(lost["track"]["rec"]["px"]["mse"]) > KR.LOST_ABOVE
    else:
        c = recs[r["constant"]]
        assert whats[r["constant"]] == KR.UNRECOVERED and c["track"]["flags"] & _capi.KF_REKEYED and c["track"]["flags"] & _capi.KF_BRIDGED
        assert c["reloc"]["rv"]["flags"] == _capi.RL_NO_CANDIDATE and c["reloc"]["n_found"] == 0 and float(c["track"]["rec"]["px"]["mse"]) > KR.LOST_ABOVE
        assert lost["reloc"]["rv"]["flags"] == _capi.RL_ATTACHED and lost["reloc"]["target"] >= 0
    assert whats[r["next"]] == KR.NOT_LOST and not nxt["track"]["flags"] & (_capi.KF_LOST | _capi.KF_RECOVERED)
    assert all(w == KR.NOT_LOST for i, w in enumerate(whats) if i not in (r["lost"], r["constant"]))


def _four(s, seed=5):
    """four cameras of `s` brought to four different situations -> the frame each is given next and its step.  Camera 0: no keyframe yet.  Camera 1: a
    frame 40 whole pixels to the right, with the true step: tracked, and below a rekey_overlap of 0.9.  Camera 2: the kidnapped frame from a zero step.
    Camera 3: a constant frame."""
    tr, _, _ = K.sequence("translation-32", seed)
    kid, _, _ = S.kidnapped(seed)
    first = K.opts(levels=S.LEVELS)
    for cam, f in ((1, tr[0]), (2, kid[0]), (3, kid[0])):
        s.push([cam], f[None])
        s.keyframe_track([cam], None, **K.opts_kw(first))
    zero = np.zeros(8, np.float32)
    return [tr[1], tr[10], kid[1], np.full((224, 320), 128, np.uint8)], [zero, np.tile(np.array([40.0, 0.0], np.float32), 4), zero, zero]


@pytest.mark.parametrize("auto_rekey", [1, 0])
def test_four_outcomes_in_one_call(fleet, tab, auto_rekey):
    """one call of four slots out of order gives each session what it gets alone, and the unlisted sessions keep every byte: FIRST, TRACKED (with a
    LOW_OVERLAP re-key under auto_rekey), lost and recovered, lost and unrecovered"""
    a, b = fleet(), fleet()
    frames, steps = _four(a)
    _four(b)
    to, ro = K.opts(levels=S.LEVELS, auto_rekey=auto_rekey, rekey_overlap=0.9, max_mse=KR.MAX_MSE), S.reloc_opts()
    alone = []
    for c in range(N_CAM):
        others = [store(b, x, S.CAPACITY) for x in range(N_CAM) if x != c]
        b.push([c], frames[c][None])
        alone.append(b.keyframe_track_recover([c], steps[c][None], hyps=tab, track=to, reloc=ro)[0])
        assert others == [store(b, x, S.CAPACITY) for x in range(N_CAM) if x != c]
    flags = [int(r["track"]["flags"]) for r in alone]
    print("alone:", flags, [int(r["reloc"]["rv"]["flags"]) for r in alone], [int(r["reloc"]["target"]) for r in alone])
    rekey = _capi.KF_REKEYED if auto_rekey else 0
    assert flags[0] == _capi.KF_FIRST | _capi.KF_REKEYED
    assert flags[1] == ((_capi.KF_LOW_OVERLAP | rekey) if auto_rekey else 0)
    assert flags[2] == _capi.KF_MSE_ABOVE_MAX | _capi.KF_BRIDGED | _capi.KF_RECOVERED and alone[2]["reloc"]["rv"]["flags"] == _capi.RL_RETRACKED
    assert flags[3] & _capi.KF_LOST and flags[3] & _capi.KF_REKEYED == rekey and not flags[3] & _capi.KF_RECOVERED
    assert alone[3]["reloc"]["rv"]["flags"] == _capi.RL_NO_CANDIDATE and alone[3]["reloc"]["n_searched"] >= 1
    assert alone[0]["reloc"].tobytes() == zero_reloc().tobytes() and alone[1]["reloc"].tobytes() == zero_reloc().tobytes()
    order = [2, 0, 3, 1]
    a.push(order, np.stack([frames[c] for c in order]))
    out = a.keyframe_track_recover(order, np.stack([steps[c] for c in order]), hyps=tab, track=to, reloc=ro)
    for i, c in enumerate(order):
        assert out[i].tobytes() == alone[c].tobytes(), c
        assert store(a, c, S.CAPACITY) == store(b, c, S.CAPACITY), c


def test_nan_step_under_the_identity_entry(fleet):
    """a NaN step on a frame moved by (16, -8) px, with hyps == NULL and n_hyp == 0 (the identity entry alone): NO_START | RECOVERED, RETRACKED with a
    search score of 1"""
    L = _capi.lib()
    cv = S.wide_canvas(5)
    key, moved = S.render_wide(cv, np.zeros(8)), S.render_wide(cv, np.tile(np.array([16.0, -8.0]), 4))
    s = fleet(capacity=0)
    s.push([1], key[None])
    s.keyframe_track([1], None, **K.opts_kw(K.opts(levels=S.LEVELS)))
    s.push([1], moved[None])
    o = KR.recover_opts(K.opts(levels=S.LEVELS, max_mse=KR.MAX_MSE), S.reloc_opts())
    ids, step, out = np.array([1], np.int32), np.full(8, np.nan, np.float32), np.zeros(1, KR.RECOVER)
    assert L.hnet_sessions_keyframe_track_recover(s._s, 1, ids.ctypes.data, step.ctypes.data, C.addressof(o), None, 0, out.ctypes.data) == 0
    t, r = out[0]["track"], out[0]["reloc"]
    assert t["flags"] == _capi.KF_NO_START | _capi.KF_RECOVERED and np.isnan(t["start_px"]).all()
    assert r["rv"]["flags"] == _capi.RL_RETRACKED and r["target"] == _capi.RL_TARGET_HELD and r["search"]["hyp"] == 0 and r["search"]["n_scored"] == 1
    assert abs(r["search"]["base"]["score"] - 1.0) <= 2.0 ** -50       # (equal thumbnails on the overlap: 1 up to the rounding of the quotient)
    assert (r["search"]["base"]["dx"], r["search"]["base"]["dy"]) == (2, -1)
    assert S.worst_px(r["rv"]["key_px"], np.tile(np.array([16.0, -8.0]), 4)) < 0.05
    assert s.keyframe(1).tobytes() == key.tobytes()
    nxt = s.keyframe_track([1], None, **K.opts_kw(K.opts(levels=S.LEVELS, max_mse=KR.MAX_MSE)))[0]      # (the same frame again: GAP, and tracked)
    assert not nxt["flags"] & _capi.KF_LOST


def test_read_only(fleet, tab):
    """two identical fleets with identical pushes and infers, one tracking with the recovery and one without: means, covariances, counts, stamps, sequence
    numbers and hnet_sessions_last_timing are equal byte for byte, and a relocalise and a revisit are accepted right after the call"""
    frames, _, steps = K.sequence("out-and-back", 5)
    a, b = fleet(), fleet()
    ids = [1, 3]
    to, ro = K.opts(max_mse=KR.MAX_MSE), S.reloc_opts()
    for i in range(4):
        f = np.stack([frames[i], frames[i + 1]])
        if i == 3:
            f[1] = 128                                 # camera 3 ends lost and unrecovered
        for s in (a, b):
            s.push(ids, f, t=[float(i), float(i)])
        st = np.stack([steps[i], steps[i + 1]])
        timing = a.last_timing()
        ra = a.keyframe_track_recover(ids, st, hyps=tab, track=to, reloc=ro)
        assert a.last_timing() == timing and a.last_keyframe_device_ms() > 0.0
        rb = b.keyframe_track(ids, st, **K.opts_kw(to))
        assert ra["track"].tobytes() == rb.tobytes()
        if i == 0:
            continue
        prior = st.astype(np.float64)
        ma, ca = a.infer(ids, prior)
        mb, cb = b.infer(ids, prior)
        assert ma.tobytes() == mb.tobytes() and ca.tobytes() == cb.tobytes()
        for c in range(N_CAM):
            assert (a.seq(c), a.image_count(c), a.latest_time(c)) == (b.seq(c), b.image_count(c), b.latest_time(c))
            assert a.image_count(c) == 0 or (a.frame(c, 0).tobytes(), a.frame(c, 1).tobytes()) == (b.frame(c, 0).tobytes(), b.frame(c, 1).tobytes())
    assert ra["track"]["flags"][0] & _capi.KF_LOST == 0 and ra["track"]["flags"][1] & _capi.KF_LOST and not ra["track"]["flags"][1] & _capi.KF_RECOVERED
    assert len(a.keyframe_relocalise(ids, **S.reloc_kw(ro))) == 2 and len(a.keyframe_revisit(ids)) == 2      # the bookkeeping moved as a track moves it


def test_refusals_change_nothing(fleet, oref, tab):
    """a call before enable, null arguments, a bad field in either option block, a table of 65 entries, a null table with n_hyp > 0, a non-finite entry,
    n < 1, a repeated id, n > max_batch and a session without an image: each returns its code, writes nothing and changes nothing - the next records are
    those of a fleet that never saw the refused calls"""
    L = _capi.lib()
    frames, _, _ = S.kidnapped(2)
    never, a, b = fleet(keyframes=False), fleet(capacity=0), fleet(capacity=0)
    out = np.full(9 * KR.RECOVER.itemsize, 0xA5, np.uint8)
    keep = out.copy()
    big = np.zeros(65, O.HYP)
    big[:] = O.table(oref, *O.IDENTITY)[0]
    good = KR.recover_opts(K.opts(levels=S.LEVELS, max_mse=KR.MAX_MSE), S.reloc_opts())

    def call(s, ids, o, t=tab, n_hyp=60, outp=out.ctypes.data):
        ids = np.asarray(ids, np.int32)
        return L.hnet_sessions_keyframe_track_recover(s._s, len(ids), ids.ctypes.data, None, C.addressof(o) if o is not None else None,
                                                      t.ctypes.data if t is not None else None, n_hyp, outp)
    never.push([0], frames[:1])
    assert call(never, [0], good) == INVALID
    for s in (a, b):
        s.push([0, 1], frames[:2])
        s.keyframe_track([0, 1], None, **K.opts_kw(K.opts(levels=S.LEVELS)))
        s.push([0], frames[1:2])
    assert call(a, [0, 0], good) == INVALID and call(a, [4], good) == INVALID and call(a, [], good) == INVALID and call(a, [-1], good) == INVALID
    assert call(a, [0, 1, 2, 3, 0, 1, 2, 3, 0], good) == CAPACITY
    assert call(a, [0, 2], good) == NOT_READY                             # camera 2 has no image
    for bad in (dict(levels=0), dict(levels=5), dict(auto_rekey=2), dict(max_age=-1), dict(rekey_overlap=1.5), dict(max_mse=-1.0), dict(huber_k=-1.0)):
        assert call(a, [0], KR.recover_opts(K.opts(**bad), S.reloc_opts())) == INVALID, bad
    for bad in (dict(levels=0), dict(min_overlap=1.5), dict(max_mse=-1.0), dict(max_closure_px=float("nan")), dict(max_iterations=33),
                dict(search=S.search_opts(radius_x=31)), dict(search=S.search_opts(min_margin=float("nan")))):
        assert call(a, [0], KR.recover_opts(K.opts(), S.reloc_opts(**bad))) == INVALID, bad
    assert call(a, [0], good, t=big, n_hyp=65) == INVALID and call(a, [0], good, t=None, n_hyp=3) == INVALID and call(a, [0], good, t=big, n_hyp=0) == INVALID
    assert call(a, [0], good, t=big, n_hyp=-1) == INVALID
    for field, k, v in (("a", 1, np.nan), ("a", 2, -np.inf), ("b", 3, 2 * 65536 + 1)):
        t = tab[:4].copy()
        t[field][2][k] = v
        assert call(a, [0], good, t=t, n_hyp=4) == INVALID, (field, k, v)
    assert call(a, [0], good, outp=None) == INVALID and call(a, [0], None) == INVALID
    assert L.hnet_sessions_keyframe_track_recover(None, 1, None, None, None, None, 0, None) == INVALID
    assert out.tobytes() == keep.tobytes()
    ra = a.keyframe_track_recover([0], None, hyps=tab, track=good.track, reloc=good.reloc)
    rb = b.keyframe_track_recover([0], None, hyps=tab, track=good.track, reloc=good.reloc)
    assert ra.tobytes() == rb.tobytes() and ra["track"]["flags"][0] & _capi.KF_RECOVERED and ra["reloc"]["rv"]["flags"][0] == _capi.RL_RETRACKED
    for s in (a, b):
        s.push([0, 1], frames[1:3])
    ta, tb = (s.keyframe_track([0, 1], None, **K.opts_kw(K.opts(levels=S.LEVELS))) for s in (a, b))
    assert ta.tobytes() == tb.tobytes()
