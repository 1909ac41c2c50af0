"""The relocalisation of a session among its keyframes on the device (include/hnet.h hnet_sessions_keyframe_relocalise; csrc/kernels_photo_search.hip;
DESIGN 7r): the kidnapped rows against their CPU-fixed gates, the pinned identity with hnet_op_photo_search, hnet_op_photo_align_robust and the host
headers, four different outcomes in one call, read-only for everything the sessions had before, and the refusals.  4 levels, 6 trials; sessions objects
of 4 cameras on a context of max_batch 8, capacity 3.

As in tests/test_gpu_keyframe_map.py "the host headers" are include/hnet_keyframe.h, include/hnet_keyframe_map.h, include/hnet_photo_search.h and
include/hnet_keyframe_reloc.h run on the host (tests/cpp/photo_search_ref.cpp) on the alignment records of the device: the search is integers and the
decisions are the same functions, so that comparison holds byte for byte, while the host's own alignment sums in another order."""
import ctypes as C

import numpy as np
import pytest

import keyframe_map_util as M
import keyframe_util as K
import photo_search_util as S
from cuahn_vio_amd import _capi, synth

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, CAPACITY = 1, 4, 5
N_CAM = 4
RELOC = S.reloc_opts()
RELOC_KW = S.reloc_kw(RELOC)
TIGHT = S.reloc_opts(max_closure_px=1e-3)
TIGHT_KW = S.reloc_kw(TIGHT)
KIDNAP = K.opts(**S.KIDNAP_TRACK)


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return S.build_ref(tmp_path_factory.mktemp("photo_search_ref_reloc_gpu"))


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


class Mirror(S.RefRelocSession):
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

    def __init__(self, s, cam, lib, capacity):
        self.s, self.cam, self.mir = s, cam, Mirror(lib, capacity)

    def track(self, frame, step, o):
        self.s.push([self.cam], frame[None])
        out = self.s.keyframe_track([self.cam], None if step is None else step[None], **K.opts_kw(o))[0]
        want = self.mir.track(out, frame, step, o)
        assert out.tobytes() == want.tobytes(), (out["flags"], want["flags"])
        return out

    def relocalise(self, frame, o):
        out = self.s.keyframe_relocalise([self.cam], **S.reloc_kw(o))[0]
        want = self.mir.relocalise(frame, o, given=out["rv"]["rec"])
        assert out.tobytes() == want.tobytes(), (out["rv"]["flags"], want["rv"]["flags"], out["target"], want["target"])
        assert self.mir.same_as(self.s, self.cam)
        return out


def _pinned(eng, out, candidate, frame, o):
    """the search record is hnet_op_photo_search's and the level-0 record hnet_op_photo_align_robust's from the searched start, byte for byte"""
    assert out["search"].tobytes() == eng.op_photo_search(candidate[None], frame[None], **S.search_kw(o.search))[0].tobytes()
    rec = eng.op_photo_align_robust(candidate[None], frame[None], out["search"]["start_px"][None], levels=o.levels, max_iterations=S.TRIALS)
    assert out["rv"]["rec"].tobytes() == rec[0].tobytes() and out["rv"]["start_px"].tobytes() == out["search"]["start_px"].tobytes()


@pytest.mark.parametrize("capacity", [0, S.CAPACITY])
@pytest.mark.parametrize("seed", S.SEEDS)
def test_kidnapped(eng, fleet, sref, seed, capacity):
    """the keyframe at the origin view, then one frame (96, -56) px away with 5 px corner offsets: the track from a zero step at 4 levels is LOST or ends
    more than 3 gates from the truth; the relocalise on the same frame is RETRACKED on the held keyframe with key_px within the gate of the true offsets;
    the next track, with the true step, is TRACKED.  Without a map and with one (the held keyframe's own slot is no candidate)."""
    cam = Cam(fleet(capacity), 2, sref, capacity)
    frames, poses, _ = S.kidnapped(seed)
    lost, rl, nxt = S.run_kidnapped(seed, cam.track, cam.relocalise)
    e_lost, e_rl = S.worst_px(lost["key_px"], poses[1]), S.worst_px(rl["rv"]["key_px"], poses[1])
    print(f"kidnapped, seed {seed}, capacity {capacity}, device: track flags {lost['flags']} at {e_lost:.2f} px; relocalise flags {rl['rv']['flags']} at "
          f"{e_rl:.4f} px (gate {S.GATE_KIDNAPPED:.4f}); {cam.s.last_keyframe_device_ms():.3f} ms on device")
    assert (lost["flags"] & _capi.KF_LOST) or e_lost > S.BEFORE_RATIO * S.GATE_KIDNAPPED
    assert rl["rv"]["flags"] == _capi.RL_RETRACKED and rl["target"] == _capi.RL_TARGET_HELD and (rl["n_searched"], rl["n_found"]) == (1, 1)
    assert e_rl <= S.GATE_KIDNAPPED
    _pinned(eng, rl, frames[0], frames[1], RELOC)
    assert not (nxt["flags"] & _capi.KF_LOST) and S.worst_px(nxt["key_px"], poses[2]) <= S.GATE_KIDNAPPED


@pytest.mark.parametrize("seed", S.SEEDS)
def test_kidnapped_with_a_map(eng, fleet, sref, seed):
    """out-and-back with max_age = 1 whose frame 4 is constant (a bridged re-key), then a frame far from the bridge's prediction but near frame 0's view:
    the relocalise attaches slot 0, h_origin_curr is within the gate of the true pose where "before" is at least 3 gates off, and the record equals the
    host headers on the device's alignment record byte for byte (Cam.relocalise)"""
    cam = Cam(fleet(), 1, sref, S.CAPACITY)
    frames, _, pose = S.kidnapped_map(seed)
    far, rl = S.run_kidnapped_map(seed, cam.track, cam.relocalise)
    b, a = M.worst_px(rl["rv"]["h_origin_before"], pose), M.worst_px(rl["rv"]["h_origin_curr"], pose)
    print(f"kidnapped with a map, seed {seed}, device: searched {rl['n_searched']}, found {rl['n_found']}; corners of h_origin_curr {b:.3f} px off the truth "
          f"before, {a:.4f} px after (gate {S.GATE_KIDNAPPED_MAP:.4f}); {cam.s.last_keyframe_device_ms():.3f} ms on device")
    assert far["flags"] & _capi.KF_LOST
    assert rl["rv"]["flags"] == _capi.RL_ATTACHED and rl["target"] == 0 and rl["rv"]["slot"] == 0 and rl["rv"]["links"] == 0
    assert a <= S.GATE_KIDNAPPED_MAP and b >= S.BEFORE_RATIO * S.GATE_KIDNAPPED_MAP
    _pinned(eng, rl, frames[0], frames[5], RELOC)
    entries, mstate = cam.s.keyframe_map_info(1)
    assert cam.s.keyframe(1).tobytes() == frames[0].tobytes() and mstate["cur_slot"][0] == 0 and mstate["cur_links"][0] == 0
    assert rl["rv"]["h_origin_curr"].tobytes() != rl["rv"]["h_origin_before"].tobytes()


def _four(s, sref, seed=5):
    """four cameras of `s` brought to four different situations -> (cams, the frame each holds).  Camera 0: an unrelated frame.  Camera 1: a frame that is
    the keyframe's view moved by whole multiples of 8 px: the alignment starts on the truth and stays.  Camera 2: the kidnapped-with-a-map sequence with
    a last frame 16 x -8 px from frame 0's view.  Camera 3: the kidnapped frame with its sub-pixel corner offsets."""
    cams = [Cam(s, c, sref, S.CAPACITY) for c in range(N_CAM)]
    key, _, _, other = S.cases(seed)
    kid, _, _ = S.kidnapped(seed)
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


def test_four_outcomes_in_one_call(fleet, sref):
    """one call of four slots out of order, max_closure_px = 1e-3, gives each session what it gets alone, and an unlisted session keeps everything:
    NO_CANDIDATE on an unrelated frame, RETRACKED, ATTACHED to slot 0, and rejected with CLOSURE_ABOVE_MAX"""
    a, b = fleet(), fleet()
    cams_a, frames = _four(a, sref)
    cams_b, _ = _four(b, sref)
    alone = []
    for c in range(N_CAM):
        others = [(b.keyframe(x).tobytes(), b.keyframe_map_info(x)[0].tobytes(), b.keyframe_map_info(x)[1].tobytes()) for x in range(N_CAM) if x != c]
        alone.append(cams_b[c].relocalise(frames[c], TIGHT))
        assert others == [(b.keyframe(x).tobytes(), b.keyframe_map_info(x)[0].tobytes(), b.keyframe_map_info(x)[1].tobytes()) for x in range(N_CAM) if x != c]
    flags = [int(r["rv"]["flags"]) for r in alone]
    print("alone:", flags, [int(r["target"]) for r in alone], [float(r["search"]["score"]) for r in alone])
    assert flags == [_capi.RL_NO_CANDIDATE, _capi.RL_RETRACKED, _capi.RL_ATTACHED, _capi.RL_CLOSURE_ABOVE_MAX]
    assert [int(r["target"]) for r in alone] == [_capi.RL_TARGET_NONE, _capi.RL_TARGET_HELD, 0, _capi.RL_TARGET_HELD]
    order = [2, 0, 3, 1]
    out = a.keyframe_relocalise(order, **TIGHT_KW)
    for i, c in enumerate(order):
        assert out[i].tobytes() == alone[c].tobytes(), c
        assert a.keyframe(c).tobytes() == b.keyframe(c).tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a.keyframe_map_info(c), b.keyframe_map_info(c)))
    again = a.keyframe_relocalise([0, 3], **TIGHT_KW)                     # a rejected and a candidate-less call changed nothing: the same records again
    assert again[0].tobytes() == alone[0].tobytes() and again[1].tobytes() == alone[3].tobytes()


def test_read_only(fleet):
    """two identical fleets with identical pushes, tracks and infers, one with (rejected) relocalises between them: means, covariances, counts, stamps,
    sequence numbers, hnet_sessions_last_timing and the track records are equal byte for byte"""
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
        rl = a.keyframe_relocalise(ids[::-1], **TIGHT_KW)
        assert a.last_timing() == timing and a.last_keyframe_device_ms() > 0.0
        assert (rl["rv"]["flags"] & (_capi.RL_REJECTED | _capi.RL_NO_CANDIDATE)).all(), rl["rv"]["flags"]
        prior = np.stack([steps[i], steps[i + 1]]).astype(np.float64)
        ma, ca = a.infer(ids, prior)
        a.keyframe_relocalise([3], **TIGHT_KW)
        mb, cb = b.infer(ids, prior)
        assert ma.tobytes() == mb.tobytes() and ca.tobytes() == cb.tobytes()
        for c in range(N_CAM):
            assert (a.seq(c), a.image_count(c), a.latest_time(c)) == (b.seq(c), b.image_count(c), b.latest_time(c))


def test_refusals_change_nothing(fleet):
    """a call before enable, null arguments, a repeated id, n > max_batch, a session without a keyframe or with an image its last track did not see, every
    option out of range: each returns its code, writes nothing and changes nothing - the next records are those of a fleet that never saw the refused calls"""
    L = _capi.lib()
    frames, _, _ = S.kidnapped(2)
    never, a, b = fleet(keyframes=False), fleet(capacity=0), fleet(capacity=0)
    out = np.full(9 * S.RELOC.itemsize, 0xA5, np.uint8)
    keep = out.copy()

    def call(s, ids, o, outp=out.ctypes.data):
        ids = np.asarray(ids, np.int32)
        return L.hnet_sessions_keyframe_relocalise(s._s, len(ids), ids.ctypes.data, C.addressof(o) if o is not None else None, outp)
    never.push([0], frames[:1])
    assert call(never, [0], RELOC) == INVALID
    for s in (a, b):
        s.push([0, 1], frames[:2])
        s.keyframe_track([0, 1], None, **K.opts_kw(KIDNAP))
        s.push([0], frames[1:2])
        s.keyframe_track([0], None, **K.opts_kw(KIDNAP))
        s.push([1, 2], frames[1:3])
    assert call(a, [0, 0], RELOC) == INVALID and call(a, [4], RELOC) == INVALID and call(a, [], RELOC) == INVALID
    assert call(a, [0, 1, 2, 3, 0, 1, 2, 3, 0], RELOC) == CAPACITY
    assert call(a, [0, 1], RELOC) == NOT_READY                            # camera 1: an image its last track did not see
    assert call(a, [2], RELOC) == NOT_READY and call(a, [3], RELOC) == NOT_READY      # no keyframe; no image
    for bad in (dict(levels=0), dict(levels=5), dict(min_overlap=1.5), dict(max_mse=-1.0), dict(max_closure_px=-1.0), dict(huber_k=-1.0), dict(max_iterations=33)):
        assert call(a, [0], S.reloc_opts(**bad)) == INVALID, bad
    for bad in (dict(radius_x=31), dict(radius_y=-1), dict(min_overlap=15), dict(min_overlap=1121), dict(min_score=1.5), dict(min_margin=float("nan"))):
        assert call(a, [0], S.reloc_opts(search=S.search_opts(**bad))) == INVALID, bad
    assert call(a, [0], RELOC, outp=None) == INVALID and call(a, [0], None) == INVALID
    assert L.hnet_sessions_keyframe_relocalise(None, 1, None, None, None) == INVALID
    assert out.tobytes() == keep.tobytes()
    ra, rb = a.keyframe_relocalise([0], **RELOC_KW), b.keyframe_relocalise([0], **RELOC_KW)
    assert ra.tobytes() == rb.tobytes() and ra["rv"]["flags"][0] == _capi.RL_RETRACKED
    ta, tb = a.keyframe_track([0, 1], None, **K.opts_kw(KIDNAP)), b.keyframe_track([0, 1], None, **K.opts_kw(KIDNAP))
    assert ta.tobytes() == tb.tobytes()
