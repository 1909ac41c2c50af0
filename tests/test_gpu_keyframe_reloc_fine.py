"""The relocalisation with the fine stage on the picked candidate on the device (include/hnet.h hnet_sessions_keyframe_relocalise_fine;
csrc/kernels_photo_search_fine.hip): the kidnapped-and-turned rows under the 30 x 12 degree table against 7s's CPU-fixed gates; the pinned
identity with hnet_op_photo_search_oriented, hnet_op_photo_search_fine, hnet_op_photo_align_robust and the host headers; four different outcomes in one
call; read-only for everything the sessions had before; the refusals; and the three existing relocalising calls, which give the bytes of a store that
never made a fine call.  4 levels, 6 trials; sessions objects of 4 cameras on a context of max_batch 8, capacity 3.

"The host headers" are the shared headers run on the host (tests/cpp/photo_search_fine_ref.cpp) on the alignment records of the device: the searches are
integers and the decisions are the same functions, so that comparison holds byte for byte, while the host's own alignment sums in another order."""
import ctypes as C

import numpy as np
import pytest

import keyframe_map_util as M
import keyframe_util as K
import photo_search_fine_util as F
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
def fref(tmp_path_factory):
    return F.build_ref(tmp_path_factory.mktemp("photo_search_fine_ref_reloc_gpu"))


class Tables:
    def __init__(self, lib, table=F.TABLE_30, **fkw):
        self.hyps, self.fo = O.yaw_table(lib, *table), F.fine_opts(lib, **fkw)
        self.fine = F.fine_yaw_table(lib, *table, self.fo.n_fine)
        self.kw = dict(hyps=self.hyps, fine=self.fine, fine_opts=F.fine_kw(self.fo))


@pytest.fixture(scope="module")
def tabs(fref):
    return Tables(fref)


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


class Mirror(F.RefSession):
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

    def __init__(self, s, cam, lib, capacity, tabs):
        self.s, self.cam, self.mir, self.t = s, cam, Mirror(lib, capacity), tabs

    def track(self, frame, step, o):
        self.s.push([self.cam], frame[None])
        out = self.s.keyframe_track([self.cam], None if step is None else step[None], **K.opts_kw(o))[0]
        want = self.mir.track(out, frame, step, o)
        assert out.tobytes() == want.tobytes(), (out["flags"], want["flags"])
        return out

    def relocalise(self, frame, o):
        out = self.s.keyframe_relocalise_fine([self.cam], **self.t.kw, **S.reloc_kw(o))[0]
        want = self.mir.relocalise_fine(frame, o, self.t.hyps, self.t.fo, self.t.fine, given=out["base"]["rv"]["rec"])
        assert out.tobytes() == want.tobytes(), (out["base"]["rv"]["flags"], want["base"]["rv"]["flags"], out["base"]["target"], want["base"]["target"],
                                                 out["fine"][["flags", "j", "ex", "ey"]], want["fine"][["flags", "j", "ex", "ey"]])
        assert self.mir.same_as(self.s, self.cam)
        return out


def _pinned(eng, out, candidate, frame, o, t):
    """the coarse part is hnet_op_photo_search_oriented's, the fine part hnet_op_photo_search_fine's and the level-0 record hnet_op_photo_align_robust's
    from the final start, byte for byte"""
    assert out["base"]["search"].tobytes() == eng.op_photo_search_oriented(candidate[None], frame[None], hyps=t.hyps, **S.search_kw(o.search))[0].tobytes()
    assert out["fine"].tobytes() == eng.op_photo_search_fine(candidate[None], frame[None], **t.kw, **S.search_kw(o.search))[0]["fine"].tobytes()
    start = out["fine"]["start_px"]
    rec = eng.op_photo_align_robust(candidate[None], frame[None], start[None], levels=o.levels, max_iterations=S.TRIALS)
    assert out["base"]["rv"]["rec"].tobytes() == rec[0].tobytes() and out["base"]["rv"]["start_px"].tobytes() == start.tobytes()


@pytest.mark.parametrize("capacity", [0, S.CAPACITY])
@pytest.mark.parametrize("seed", S.SEEDS)
def test_kidnapped_and_turned(eng, fleet, fref, tabs, seed, capacity):
    """7s's kidnapped-and-turned row under the 30 x 12 degree table: the fine relocalise is RETRACKED on the held keyframe with key_px within 7s's gate of
    the true offsets, from a REFINED start closer to the truth than the coarse one, and the next track, with the true step, is TRACKED"""
    cam = Cam(fleet(capacity), 2, fref, capacity, tabs)
    frames, poses, _ = O.turned(seed)
    lost, rl, nxt = O.run_turned(seed, cam.track, cam.relocalise)
    b, p = rl["base"], rl["fine"]
    e_rl = S.worst_px(b["rv"]["key_px"], poses[1])
    ec, ef = S.worst_px(b["search"]["base"]["start_px"], poses[1]), S.worst_px(p["start_px"], poses[1])
    print(f"kidnapped and turned, 30 x 12, seed {seed}, capacity {capacity}, device: coarse start {ec:.2f} px, fine start {ef:.2f} px; relocalise flags "
          f"{b['rv']['flags']} at {e_rl:.4f} px (gate {O.GATE_TURNED:.4f}); {cam.s.last_keyframe_device_ms():.3f} ms on device")
    assert p["flags"] == _capi.PSF_REFINED and ef < ec and ef < O.BASIN_PX
    assert b["rv"]["flags"] == _capi.RL_RETRACKED and b["target"] == _capi.RL_TARGET_HELD and (b["n_searched"], b["n_found"]) == (1, 1)
    assert e_rl <= O.GATE_TURNED
    _pinned(eng, rl, frames[0], frames[1], TURNED, tabs)
    assert not (nxt["flags"] & _capi.KF_LOST) and S.worst_px(nxt["key_px"], poses[2]) <= O.GATE_TURNED


@pytest.mark.parametrize("seed", S.SEEDS)
def test_kidnapped_and_turned_with_a_map(eng, fleet, fref, tabs, seed):
    """7s's row with a map under the 30 x 12 degree table: the fine relocalise attaches a stored keyframe, h_origin_curr is within 7s's gate of the true
    pose, and the record equals the host headers on the device's alignment record byte for byte"""
    cam = Cam(fleet(), 1, fref, S.CAPACITY, tabs)
    frames, _, pose = O.turned_map(seed)
    far, rl = O.run_turned_map(seed, cam.track, cam.relocalise)
    b = rl["base"]
    before, after = M.worst_px(b["rv"]["h_origin_before"], pose), M.worst_px(b["rv"]["h_origin_curr"], pose)
    print(f"kidnapped and turned with a map, 30 x 12, seed {seed}, device: searched {b['n_searched']}, found {b['n_found']}, target {b['target']}; fine flags "
          f"{rl['fine']['flags']}; h_origin_curr {before:.3f} px off before, {after:.4f} px after (gate {O.GATE_TURNED_MAP:.4f}); "
          f"{cam.s.last_keyframe_device_ms():.3f} ms on device")
    slot = int(b["target"])
    assert far["flags"] & _capi.KF_LOST and rl["fine"]["flags"] == _capi.PSF_REFINED
    assert b["rv"]["flags"] == _capi.RL_ATTACHED and slot >= 0 and b["rv"]["slot"] == slot
    assert after <= O.GATE_TURNED_MAP and before >= O.BEFORE_RATIO * O.GATE_TURNED_MAP
    _pinned(eng, rl, cam.mir.images[slot], frames[5], RELOC, tabs)
    assert cam.s.keyframe(1).tobytes() == cam.mir.images[slot].tobytes() and cam.s.keyframe_map_info(1)[1]["cur_slot"][0] == slot


def _four(s, lib, tabs, seed=5):
    """four cameras of `s` brought to four different situations -> (cams, the frame each holds).  Camera 0: an unrelated frame.  Camera 1: the keyframe's
    view moved by whole multiples of 8 px.  Camera 2: the kidnapped-with-a-map sequence with a last frame 16 x -8 px from frame 0's view.  Camera 3: the
    kidnapped-and-turned frame, whose final start lies some pixels from the truth."""
    cams = [Cam(s, c, lib, S.CAPACITY, tabs) for c in range(N_CAM)]
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


def test_four_outcomes_in_one_call(fleet, fref, tabs):
    """one call of four slots out of order, max_closure_px = 1e-3, gives each session what it gets alone, and an unlisted session keeps everything:
    NO_CANDIDATE on an unrelated frame (fine SKIPPED, NaN start), RETRACKED, ATTACHED to slot 0, and the turned frame rejected with CLOSURE_ABOVE_MAX"""
    a, b = fleet(), fleet()
    cams_a, frames = _four(a, fref, tabs)
    cams_b, _ = _four(b, fref, tabs)
    alone = []
    for c in range(N_CAM):
        others = [(b.keyframe(x).tobytes(), b.keyframe_map_info(x)[0].tobytes(), b.keyframe_map_info(x)[1].tobytes()) for x in range(N_CAM) if x != c]
        alone.append(cams_b[c].relocalise(frames[c], TIGHT))
        assert others == [(b.keyframe(x).tobytes(), b.keyframe_map_info(x)[0].tobytes(), b.keyframe_map_info(x)[1].tobytes()) for x in range(N_CAM) if x != c]
    flags = [int(r["base"]["rv"]["flags"]) for r in alone]
    print("alone:", flags, [int(r["base"]["target"]) for r in alone], [int(r["fine"]["flags"]) for r in alone], [float(r["fine"]["score"]) for r in alone])
    assert flags == [_capi.RL_NO_CANDIDATE, _capi.RL_RETRACKED, _capi.RL_ATTACHED, _capi.RL_CLOSURE_ABOVE_MAX]
    assert [int(r["base"]["target"]) for r in alone] == [_capi.RL_TARGET_NONE, _capi.RL_TARGET_HELD, 0, _capi.RL_TARGET_HELD]
    assert [int(r["fine"]["flags"]) for r in alone] == [_capi.PSF_SKIPPED] + [_capi.PSF_REFINED] * 3
    assert np.array_equal(alone[0]["fine"]["start_px"].view(np.uint32), F.NAN32) and np.array_equal(alone[0]["base"]["rv"]["start_px"].view(np.uint32), F.NAN32)
    order = [2, 0, 3, 1]
    out = a.keyframe_relocalise_fine(order, **tabs.kw, **TIGHT_KW)
    for i, c in enumerate(order):
        assert out[i].tobytes() == alone[c].tobytes(), c
        assert a.keyframe(c).tobytes() == b.keyframe(c).tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a.keyframe_map_info(c), b.keyframe_map_info(c)))
    again = a.keyframe_relocalise_fine([0, 3], **tabs.kw, **TIGHT_KW)     # a rejected and a candidate-less call changed nothing: the same records again
    assert again[0].tobytes() == alone[0].tobytes() and again[1].tobytes() == alone[3].tobytes()


def test_read_only(fleet, tabs):
    """two identical fleets with identical pushes, tracks and infers, one with (rejected) fine relocalises between them: means, covariances, counts,
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
        rl = a.keyframe_relocalise_fine(ids[::-1], **tabs.kw, **TIGHT_KW)
        assert a.last_timing() == timing and a.last_keyframe_device_ms() > 0.0
        assert (rl["base"]["rv"]["flags"] & (_capi.RL_REJECTED | _capi.RL_NO_CANDIDATE)).all(), rl["base"]["rv"]["flags"]
        prior = np.stack([steps[i], steps[i + 1]]).astype(np.float64)
        ma, ca = a.infer(ids, prior)
        a.keyframe_relocalise_fine([3], hyps=tabs.hyps[12:19], fine=tabs.fine[12:19], fine_opts=tabs.kw["fine_opts"], **TIGHT_KW)
        mb, cb = b.infer(ids, prior)
        assert ma.tobytes() == mb.tobytes() and ca.tobytes() == cb.tobytes()
        for c in range(N_CAM):
            assert (a.seq(c), a.image_count(c), a.latest_time(c)) == (b.seq(c), b.image_count(c), b.latest_time(c))


def test_refusals_change_nothing(fleet, fref, tabs):
    """the oriented relocalise's refusals, and null fine options, a null fine table, n_fine, radius and min_score out of range and an invalid fine entry:
    each returns its code, writes nothing and changes nothing - the next records are those of a fleet that never saw the refused calls"""
    L = _capi.lib()
    frames, _, _ = O.turned(2)
    never, a, b = fleet(keyframes=False), fleet(capacity=0), fleet(capacity=0)
    out = np.full(9 * F.FRELOC.itemsize, 0xA5, np.uint8)
    keep = out.copy()

    def call(s, ids, o, t=tabs.hyps, n_hyp=30, fo=tabs.fo, f=tabs.fine, outp=out.ctypes.data):
        ids = np.asarray(ids, np.int32)
        return L.hnet_sessions_keyframe_relocalise_fine(s._s, len(ids), ids.ctypes.data, C.addressof(o) if o is not None else None,
                                                        t.ctypes.data if t is not None else None, n_hyp, C.addressof(fo) if fo is not None else None,
                                                        f.ctypes.data if f is not None else None, outp)
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
    for bad in (dict(levels=0), dict(min_overlap=1.5), dict(max_closure_px=-1.0), dict(huber_k=-1.0)):
        assert call(a, [0], S.reloc_opts(**bad)) == INVALID, bad
    assert call(a, [0], S.reloc_opts(search=S.search_opts(radius_x=31))) == INVALID
    assert call(a, [0], TURNED, n_hyp=0) == INVALID and call(a, [0], TURNED, n_hyp=65) == INVALID and call(a, [0], TURNED, t=None) == INVALID
    assert call(a, [0], TURNED, fo=None) == INVALID and call(a, [0], TURNED, f=None) == INVALID
    for bad in (dict(n_fine=0), dict(n_fine=10), dict(radius=-1), dict(radius=5), dict(min_score=float("nan")), dict(min_score=1.5)):
        assert call(a, [0], TURNED, fo=F.fine_opts(fref, **bad)) == INVALID, bad
    for field, k, v in (("a", 1, np.nan), ("a", 2, -np.inf), ("b", 3, 2 * 65536 + 1), ("b", 0, -2 * 65536 - 1)):
        f = tabs.fine.copy()
        f[field][29, 4][k] = v
        assert call(a, [0], TURNED, f=f) == INVALID, (field, k, v)
    assert call(a, [0], TURNED, outp=None) == INVALID and call(a, [0], None) == INVALID
    assert L.hnet_sessions_keyframe_relocalise_fine(None, 1, None, None, None, 1, None, None, None) == INVALID
    assert out.tobytes() == keep.tobytes()
    kw = S.reloc_kw(TURNED)
    ra, rb = a.keyframe_relocalise_fine([0], **tabs.kw, **kw), b.keyframe_relocalise_fine([0], **tabs.kw, **kw)
    assert ra.tobytes() == rb.tobytes() and ra["base"]["rv"]["flags"][0] == _capi.RL_RETRACKED
    ta, tb = a.keyframe_track([0, 1], None, **K.opts_kw(KIDNAP)), b.keyframe_track([0, 1], None, **K.opts_kw(KIDNAP))
    assert ta.tobytes() == tb.tobytes()


def test_existing_calls_are_unaffected(fleet, fref, tabs):
    """after a (rejected) fine call on the same store, hnet_sessions_keyframe_relocalise, hnet_sessions_keyframe_relocalise_oriented and
    hnet_sessions_keyframe_track_recover give the bytes they give on a twin that never made one"""
    frames, _, step = O.turned(1)
    key, views, _, _ = S.cases(1)
    tab60 = O.yaw_table(fref)
    a, b = fleet(), fleet()
    ids = [0, 2]
    for s in (a, b):
        s.push(ids, np.stack([frames[0], key]))
        s.keyframe_track(ids, None, **K.opts_kw(KIDNAP))
        s.push(ids, np.stack([frames[1], views[0]]))
        s.keyframe_track(ids, None, **K.opts_kw(KIDNAP))
    rej = a.keyframe_relocalise_fine(ids, **tabs.kw, **TIGHT_KW)
    assert (rej["base"]["rv"]["flags"] & (_capi.RL_REJECTED | _capi.RL_NO_CANDIDATE)).all() and (rej["fine"]["flags"] == _capi.PSF_REFINED).any()
    pa, pb = (s.keyframe_relocalise(ids, **S.reloc_kw(TURNED)) for s in (a, b))
    assert pa.tobytes() == pb.tobytes() and (pa["rv"]["flags"] == _capi.RL_RETRACKED).any()
    a.keyframe_relocalise_fine(ids[::-1], **tabs.kw, **TIGHT_KW)
    oa, ob = (s.keyframe_relocalise_oriented(ids, hyps=tab60, **S.reloc_kw(TURNED)) for s in (a, b))
    assert oa.tobytes() == ob.tobytes() and (oa["rv"]["flags"] == _capi.RL_RETRACKED).any()
    a.keyframe_relocalise_fine(ids, **tabs.kw, **TIGHT_KW)
    for s in (a, b):
        s.push(ids, np.stack([frames[2], views[1]]))
    ra, rb = (s.keyframe_track_recover(ids, np.stack([step, np.zeros(8, np.float32)]), hyps=tab60) for s in (a, b))
    assert ra.tobytes() == rb.tobytes()
    assert all(a.keyframe(c).tobytes() == b.keyframe(c).tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a.keyframe_map_info(c), b.keyframe_map_info(c)))
               for c in ids)
