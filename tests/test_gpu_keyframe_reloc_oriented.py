"""The oriented relocalisation of a session among its keyframes on the device (include/hnet.h hnet_sessions_keyframe_relocalise_oriented;
csrc/kernels_photo_search_oriented.hip): the kidnapped-and-turned rows against their CPU-fixed gates, where the plain relocalise finds no
candidate; the pinned identity with hnet_op_photo_search_oriented, hnet_op_photo_align_robust and the host headers; four different outcomes in one call;
read-only for everything the sessions had before; and the refusals.  4 levels, 6 trials; sessions objects of 4 cameras on a context of max_batch 8,
capacity 3.

As in tests/test_gpu_keyframe_reloc.py "the host headers" are the shared headers run on the host (tests/cpp/photo_search_oriented_ref.cpp) on the alignment
records of the device: the search is integers and the decisions are the same functions, so that comparison holds byte for byte, while the host's own
alignment sums in another order."""
import ctypes as C

import numpy as np
import pytest

import keyframe_map_util as M
import keyframe_util as K
import photo_search_oriented_util as O
import photo_search_util as S
from cuahn_vio_amd import _capi, synth

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, CAPACITY = 1, 4, 5
N_CAM = 4
RELOC = S.reloc_opts()
TURNED = S.reloc_opts(min_overlap=O.TURNED_MIN_OVERLAP)
TIGHT = S.reloc_opts(max_closure_px=1e-3, min_overlap=O.TURNED_MIN_OVERLAP)
TIGHT_KW = S.reloc_kw(TIGHT)
KIDNAP = K.opts(**S.KIDNAP_TRACK)


@pytest.fixture(scope="module")
def oref(tmp_path_factory):
    return O.build_ref(tmp_path_factory.mktemp("photo_search_oriented_ref_reloc_gpu"))


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


class Mirror(O.RefSession):
    """one device session restated on the host headers, from the device's alignment records"""

    def track(self, dev, frame, step, o):
        if self.state["has_key"][0]:
            start = K.ref_compose(self.lib, np.zeros(8, np.float32) if step is None else step, self.state["key_px"][0])
            assert start is not None
        else:
            start = np.zeros(8, np.float32)
        ns, want, copy = K.ref_decide(self.lib, self.state, start, dev["rec"], o)
        if self.capacity > 0:
            slot, self.mstate, self.entries = M.ref_note(self.lib, int(want["flags"][0]), copy, ns, self.mstate, self.entries)
            if slot >= 0:
                self.images[slot] = frame
        self.state = ns
        if copy:
            self.key = np.array(frame, np.uint8)
        return want[0]

    def same_as(self, s, cam):
        ok = s.keyframe(cam).tobytes() == self.key.tobytes()
        if self.capacity > 0:
            entries, mstate = s.keyframe_map_info(cam)
            ok = ok and entries.tobytes() == self.entries.tobytes() and mstate.tobytes() == self.mstate.tobytes()
        return ok


class Cam:
    """a camera of a device fleet and its mirror"""

    def __init__(self, s, cam, lib, capacity, tab):
        self.s, self.cam, self.mir, self.tab = s, cam, Mirror(lib, capacity), tab

    def track(self, frame, step, o):
        self.s.push([self.cam], frame[None])
        out = self.s.keyframe_track([self.cam], None if step is None else step[None], **K.opts_kw(o))[0]
        want = self.mir.track(out, frame, step, o)
        assert out.tobytes() == want.tobytes(), (out["flags"], want["flags"])
        return out

    def relocalise(self, frame, o):
        out = self.s.keyframe_relocalise_oriented([self.cam], hyps=self.tab, **S.reloc_kw(o))[0]
        want = self.mir.relocalise_oriented(frame, o, self.tab, given=out["rv"]["rec"])
        assert out.tobytes() == want.tobytes(), (out["rv"]["flags"], want["rv"]["flags"], out["target"], want["target"], out["search"]["hyp"], want["search"]["hyp"])
        assert self.mir.same_as(self.s, self.cam)
        return out

    def plain_then_oriented(self, frame, o):
        """the plain relocalise finds no candidate and changes nothing; then the oriented one"""
        plain = self.s.keyframe_relocalise([self.cam], **S.reloc_kw(o))[0]
        assert plain["rv"]["flags"] == _capi.RL_NO_CANDIDATE and plain["n_found"] == 0 and self.mir.same_as(self.s, self.cam)
        return self.relocalise(frame, o)


def _pinned(eng, out, candidate, frame, o, tab):
    """the search record is hnet_op_photo_search_oriented's and the level-0 record hnet_op_photo_align_robust's from the searched start, byte for byte"""
    assert out["search"].tobytes() == eng.op_photo_search_oriented(candidate[None], frame[None], hyps=tab, **S.search_kw(o.search))[0].tobytes()
    start = out["search"]["base"]["start_px"]
    rec = eng.op_photo_align_robust(candidate[None], frame[None], start[None], levels=o.levels, max_iterations=S.TRIALS)
    assert out["rv"]["rec"].tobytes() == rec[0].tobytes() and out["rv"]["start_px"].tobytes() == start.tobytes()


@pytest.mark.parametrize("capacity", [0, S.CAPACITY])
@pytest.mark.parametrize("seed", S.SEEDS)
def test_kidnapped_and_turned(eng, fleet, oref, tab, seed, capacity):
    """the keyframe at the origin view, then one frame (96, -56) px away, turned by 33 degrees, with 5 px corner offsets: the track from a zero step ends
    more than 3 gates from the truth, the plain relocalise answers NO_CANDIDATE, the oriented one is RETRACKED on the held keyframe with key_px within
    the gate of the true offsets, and the next track, with the true step, is TRACKED.  Without a map and with one."""
    cam = Cam(fleet(capacity), 2, oref, capacity, tab)
    frames, poses, _ = O.turned(seed)
    lost, rl, nxt = O.run_turned(seed, cam.track, cam.plain_then_oriented)
    e_lost, e_rl = S.worst_px(lost["key_px"], poses[1]), S.worst_px(rl["rv"]["key_px"], poses[1])
    print(f"kidnapped and turned, seed {seed}, capacity {capacity}, device: track flags {lost['flags']} at {e_lost:.2f} px; entry {rl['search']['hyp']}; relocalise "
          f"flags {rl['rv']['flags']} at {e_rl:.4f} px (gate {O.GATE_TURNED:.4f}); {cam.s.last_keyframe_device_ms():.3f} ms on device")
    assert (lost["flags"] & _capi.KF_LOST) or e_lost > O.BEFORE_RATIO * O.GATE_TURNED
    assert rl["rv"]["flags"] == _capi.RL_RETRACKED and rl["target"] == _capi.RL_TARGET_HELD and (rl["n_searched"], rl["n_found"]) == (1, 1)
    assert e_rl <= O.GATE_TURNED
    _pinned(eng, rl, frames[0], frames[1], TURNED, tab)
    assert not (nxt["flags"] & _capi.KF_LOST) and S.worst_px(nxt["key_px"], poses[2]) <= O.GATE_TURNED


@pytest.mark.parametrize("seed", S.SEEDS)
def test_kidnapped_and_turned_with_a_map(eng, fleet, oref, tab, seed):
    """out-and-back with max_age = 1 whose frame 4 is constant (a bridged re-key), then a frame far from the bridge's prediction, near frame 0's view and
    turned by 33 degrees: the plain relocalise answers NO_CANDIDATE, the oriented one attaches a stored keyframe, h_origin_curr is within the gate of
    the true pose where "before" is at least 3 gates off, and the record equals the host headers on the device's alignment record byte for byte"""
    cam = Cam(fleet(), 1, oref, S.CAPACITY, tab)
    frames, _, pose = O.turned_map(seed)
    far, rl = O.run_turned_map(seed, cam.track, cam.plain_then_oriented)
    b, a = M.worst_px(rl["rv"]["h_origin_before"], pose), M.worst_px(rl["rv"]["h_origin_curr"], pose)
    print(f"kidnapped and turned with a map, seed {seed}, device: searched {rl['n_searched']}, found {rl['n_found']}, target {rl['target']}; corners of "
          f"h_origin_curr {b:.3f} px off the truth before, {a:.4f} px after (gate {O.GATE_TURNED_MAP:.4f}); {cam.s.last_keyframe_device_ms():.3f} ms on device")
    assert far["flags"] & _capi.KF_LOST
    slot = int(rl["target"])
    assert rl["rv"]["flags"] == _capi.RL_ATTACHED and slot >= 0 and rl["rv"]["slot"] == slot
    assert a <= O.GATE_TURNED_MAP and b >= O.BEFORE_RATIO * O.GATE_TURNED_MAP
    candidate = cam.mir.images[slot]
    _pinned(eng, rl, candidate, frames[5], RELOC, tab)
    entries, mstate = cam.s.keyframe_map_info(1)
    assert cam.s.keyframe(1).tobytes() == candidate.tobytes() and mstate["cur_slot"][0] == slot
    assert rl["rv"]["h_origin_curr"].tobytes() != rl["rv"]["h_origin_before"].tobytes()


def _four(s, oref, tab, seed=5):
    """four cameras of `s` brought to four different situations -> (cams, the frame each holds).  Camera 0: an unrelated frame.  Camera 1: a frame that is
    the keyframe's view moved by whole multiples of 8 px: the identity entry wins, the alignment starts on the truth and stays.  Camera 2: the
    kidnapped-with-a-map sequence with a last frame 16 x -8 px from frame 0's view.  Camera 3: the kidnapped-and-turned frame: its start is a table
    entry's, some pixels from the truth."""
    cams = [Cam(s, c, oref, S.CAPACITY, tab) for c in range(N_CAM)]
    key, _, _, other = S.cases(seed)
    kid, _, _ = O.turned(seed)
    whole = S.render_wide(S.wide_canvas(seed), np.tile(np.array([-96.0, 56.0]), 4))
    cams[0].track(key, None, KIDNAP)
    cams[0].track(other, None, KIDNAP)
    cams[1].track(key, None, KIDNAP)
    cams[1].track(whole, None, KIDNAP)
    mf, steps, _ = S.kidnapped_map(seed)
    near = K.render(synth.canvas(seed), np.tile(np.array([16.0, -8.0]), 4))
    for i in range(5):
        cams[2].track(mf[i], steps[i], K.opts(**M.TRACK_OPTS))
    cams[2].track(near, None, K.opts(levels=K.LEVELS, auto_rekey=0))
    cams[3].track(kid[0], None, KIDNAP)
    cams[3].track(kid[1], None, KIDNAP)
    return cams, [other, whole, near, kid[1]]


def test_four_outcomes_in_one_call(fleet, oref, tab):
    """one call of four slots out of order, max_closure_px = 1e-3, gives each session what it gets alone, and an unlisted session keeps everything:
    NO_CANDIDATE on an unrelated frame, RETRACKED, ATTACHED to slot 0, and the turned frame rejected with CLOSURE_ABOVE_MAX"""
    a, b = fleet(), fleet()
    cams_a, frames = _four(a, oref, tab)
    cams_b, _ = _four(b, oref, tab)
    alone = []
    for c in range(N_CAM):
        others = [(b.keyframe(x).tobytes(), b.keyframe_map_info(x)[0].tobytes(), b.keyframe_map_info(x)[1].tobytes()) for x in range(N_CAM) if x != c]
        alone.append(cams_b[c].relocalise(frames[c], TIGHT))
        assert others == [(b.keyframe(x).tobytes(), b.keyframe_map_info(x)[0].tobytes(), b.keyframe_map_info(x)[1].tobytes()) for x in range(N_CAM) if x != c]
    flags = [int(r["rv"]["flags"]) for r in alone]
    print("alone:", flags, [int(r["target"]) for r in alone], [int(r["search"]["hyp"]) for r in alone], [float(r["search"]["base"]["score"]) for r in alone])
    assert flags == [_capi.RL_NO_CANDIDATE, _capi.RL_RETRACKED, _capi.RL_ATTACHED, _capi.RL_CLOSURE_ABOVE_MAX]
    assert [int(r["target"]) for r in alone] == [_capi.RL_TARGET_NONE, _capi.RL_TARGET_HELD, 0, _capi.RL_TARGET_HELD]
    assert alone[1]["search"]["hyp"] == 30 and alone[2]["search"]["hyp"] == 30 and alone[3]["search"]["hyp"] in (35, 36)
    order = [2, 0, 3, 1]
    out = a.keyframe_relocalise_oriented(order, hyps=tab, **TIGHT_KW)
    for i, c in enumerate(order):
        assert out[i].tobytes() == alone[c].tobytes(), c
        assert a.keyframe(c).tobytes() == b.keyframe(c).tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a.keyframe_map_info(c), b.keyframe_map_info(c)))
    again = a.keyframe_relocalise_oriented([0, 3], hyps=tab, **TIGHT_KW)  # a rejected and a candidate-less call changed nothing: the same records again
    assert again[0].tobytes() == alone[0].tobytes() and again[1].tobytes() == alone[3].tobytes()


def test_read_only(fleet, tab):
    """two identical fleets with identical pushes, tracks and infers, one with (rejected) oriented relocalises between them: means, covariances, counts,
    stamps, sequence numbers, hnet_sessions_last_timing and the track records are equal byte for byte"""
    frames, _, steps = K.sequence("out-and-back", 5)
    a, b = fleet(), fleet()
    ids = [1, 3]
    kw = K.opts_kw(K.opts())
    for i in range(4):
        for s in (a, b):
            s.push(ids, np.stack([frames[i], frames[i + 1]]), t=[float(i), float(i)])
        ta, tb = (s.keyframe_track(ids, np.stack([steps[i], steps[i + 1]]), **kw) for s in (a, b))
        assert ta.tobytes() == tb.tobytes()
        if i == 0:
            continue
        timing = a.last_timing()
        rl = a.keyframe_relocalise_oriented(ids[::-1], hyps=tab, **TIGHT_KW)
        assert a.last_timing() == timing and a.last_keyframe_device_ms() > 0.0
        assert (rl["rv"]["flags"] & (_capi.RL_REJECTED | _capi.RL_NO_CANDIDATE)).all(), rl["rv"]["flags"]
        prior = np.stack([steps[i], steps[i + 1]]).astype(np.float64)
        ma, ca = a.infer(ids, prior)
        a.keyframe_relocalise_oriented([3], hyps=tab[24:37], **TIGHT_KW)
        mb, cb = b.infer(ids, prior)
        assert ma.tobytes() == mb.tobytes() and ca.tobytes() == cb.tobytes()
        for c in range(N_CAM):
            assert (a.seq(c), a.image_count(c), a.latest_time(c)) == (b.seq(c), b.image_count(c), b.latest_time(c))


def test_refusals_change_nothing(fleet, oref, tab):
    """a call before enable, null arguments, a repeated id, n > max_batch, a session without a keyframe or with an image its last track did not see, an
    option out of range, a table of 0 or 65 entries, a null table, a non-finite entry and one past the scale's range: each returns its code, writes
    nothing and changes nothing - the next records are those of a fleet that never saw the refused calls"""
    L = _capi.lib()
    frames, _, _ = O.turned(2)
    never, a, b = fleet(keyframes=False), fleet(capacity=0), fleet(capacity=0)
    out = np.full(9 * O.ORELOC.itemsize, 0xA5, np.uint8)
    keep = out.copy()
    big = np.zeros(65, O.HYP)
    big[:] = O.table(oref, *O.IDENTITY)[0]

    def call(s, ids, o, t=tab, n_hyp=60, outp=out.ctypes.data):
        ids = np.asarray(ids, np.int32)
        return L.hnet_sessions_keyframe_relocalise_oriented(s._s, len(ids), ids.ctypes.data, C.addressof(o) if o is not None else None,
                                                            t.ctypes.data if t is not None else None, n_hyp, outp)
    never.push([0], frames[:1])
    assert call(never, [0], TURNED) == INVALID
    for s in (a, b):
        s.push([0, 1], frames[:2])
        s.keyframe_track([0, 1], None, **K.opts_kw(KIDNAP))
        s.push([0], frames[1:2])
        s.keyframe_track([0], None, **K.opts_kw(KIDNAP))
        s.push([1, 2], frames[1:3])
    assert call(a, [0, 0], TURNED) == INVALID and call(a, [4], TURNED) == INVALID and call(a, [], TURNED) == INVALID
    assert call(a, [0, 1, 2, 3, 0, 1, 2, 3, 0], TURNED) == CAPACITY
    assert call(a, [0, 1], TURNED) == NOT_READY                           # camera 1: an image its last track did not see
    assert call(a, [2], TURNED) == NOT_READY and call(a, [3], TURNED) == NOT_READY      # no keyframe; no image
    for bad in (dict(levels=0), dict(levels=5), dict(min_overlap=1.5), dict(max_mse=-1.0), dict(max_closure_px=-1.0), dict(huber_k=-1.0), dict(max_iterations=33)):
        assert call(a, [0], S.reloc_opts(**bad)) == INVALID, bad
    for bad in (dict(radius_x=31), dict(radius_y=-1), dict(min_overlap=15), dict(min_score=1.5), dict(min_margin=float("nan"))):
        assert call(a, [0], S.reloc_opts(search=S.search_opts(**bad))) == INVALID, bad
    assert call(a, [0], TURNED, t=big, n_hyp=0) == INVALID and call(a, [0], TURNED, t=big, n_hyp=65) == INVALID and call(a, [0], TURNED, t=None) == INVALID
    for field, k, v in (("a", 1, np.nan), ("a", 2, -np.inf), ("b", 3, 2 * 65536 + 1), ("b", 0, -2 * 65536 - 1)):
        t = tab[:4].copy()
        t[field][2][k] = v
        assert call(a, [0], TURNED, t=t, n_hyp=4) == INVALID, (field, k, v)
    assert call(a, [0], TURNED, outp=None) == INVALID and call(a, [0], None) == INVALID
    assert L.hnet_sessions_keyframe_relocalise_oriented(None, 1, None, None, None, 1, None) == INVALID
    assert out.tobytes() == keep.tobytes()
    kw = S.reloc_kw(TURNED)
    ra, rb = a.keyframe_relocalise_oriented([0], hyps=tab, **kw), b.keyframe_relocalise_oriented([0], hyps=tab, **kw)
    assert ra.tobytes() == rb.tobytes() and ra["rv"]["flags"][0] == _capi.RL_RETRACKED
    ta, tb = a.keyframe_track([0, 1], None, **K.opts_kw(KIDNAP)), b.keyframe_track([0, 1], None, **K.opts_kw(KIDNAP))
    assert ta.tobytes() == tb.tobytes()
