"""The keyframe map and the revisit on the device (include/hnet.h hnet_sessions_enable_keyframe_map, hnet_sessions_keyframe_revisit;
csrc/kernels_keyframe_map.hip): the pinned identity with hnet_op_photo_align_robust and the host header, the accuracy rows, a track that the map
does not disturb, eviction, slot hygiene, the resets, read-only for everything the sessions had before, and the refusals.  levels = 3, 6 trials;
sessions objects of 4 cameras on a context of max_batch 8, capacity 3 unless stated.

"The host reference's" state of a device session is here the MIRROR below: the functions of include/hnet_keyframe_map.h and include/hnet_keyframe.h run
on the host (tests/cpp/keyframe_map_ref.cpp), fed the alignment records of the device.  The host reference's own alignment sums in another order than
the device's (tests/test_gpu_photo_robust.py: 1e-13 relative on the sums), so the doubles of its records are not the device's byte for byte, while every
function of the two headers is: the mirror is the comparison that can hold byte for byte.  test_pinned_identity also compares with the session that is
wholly on the host: integers equal, offsets within that file's bound."""
import ctypes as C

import numpy as np
import pytest

import keyframe_map_util as M
import keyframe_util as K
import photo_align_util as U
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, CAPACITY = 1, 4, 5
N_CAM = 4
OFFSETS_VS_REFERENCE_PX = 1e-4             # offsets, device against the host reference's own alignment: the bound of tests/test_gpu_photo_robust.py
FIRST = _capi.KF_FIRST | _capi.KF_REKEYED
TRACK = K.opts(**M.TRACK_OPTS)
TRACK_KW = K.opts_kw(TRACK)


@pytest.fixture(scope="module")
def mref(tmp_path_factory):
    return M.build_ref(tmp_path_factory.mktemp("keyframe_map_ref_gpu"))


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

    def make(capacity=M.CAPACITY, keyframes=True):
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


class Mirror:
    """one device session restated on the host header: state, keyframe, entries, map state and images, from the device's alignment records"""

    def __init__(self, lib, capacity=M.CAPACITY):
        self.lib, self.state, self.key = lib, K.new_state(), np.zeros((224, 320), np.uint8)
        self.entries, self.mstate = M.new_map(capacity)
        self.images = np.zeros((capacity, 224, 320), np.uint8)

    def track(self, dev, frame, step, o):
        """dev: the device's record of this track -> the record the header gives on the device's alignment record; the map is updated"""
        if self.state["has_key"][0]:
            start = K.ref_compose(self.lib, np.zeros(8, np.float32) if step is None else step, self.state["key_px"][0])
            assert start is not None
        else:
            start = np.zeros(8, np.float32)
        ns, want, copy = K.ref_decide(self.lib, self.state, start, dev["rec"], o)
        slot, self.mstate, self.entries = M.ref_note(self.lib, int(want["flags"][0]), copy, ns, self.mstate, self.entries)
        self.state = ns
        assert (slot >= 0) == bool(copy)
        if copy:
            self.key = np.array(frame, np.uint8)
            self.images[slot] = frame
        return want[0]

    def revisit(self, hb, slot, grid, start, rec, o):
        """rec: the alignment's record of the candidate -> the record the header gives; states, keyframe updated on an attach"""
        self.state, self.mstate, want, attach = M.ref_decide(self.lib, self.state, self.mstate, self.entries, slot, grid, start, hb, rec, o)
        if attach:
            self.key = self.images[slot].copy()
        return want[0], attach

    def same_map(self, s, cam):
        entries, mstate = s.keyframe_map_info(cam)
        return entries.tobytes() == self.entries.tobytes() and mstate.tobytes() == self.mstate.tobytes()


def _images(s, cam, capacity=M.CAPACITY):
    return np.stack([s.map_keyframe(cam, j) for j in range(capacity)])


@pytest.mark.parametrize("name", list(M.ROWS))
def test_pinned_identity(eng, fleet, mref, name):
    """a row on one camera (seed 1, n = 1 calls).  On the revisit: rec equals hnet_op_photo_align_robust(map keyframe downloaded before the call, curr,
    start_px) byte for byte; slot, grid count and start_px equal the host header's select on the downloaded map_info; the whole record equals the host
    header's decide_revisit byte for byte.  After the attach: get_keyframe equals the map image, map_info the mirror's, the next two tracks' records the
    mirror's byte for byte.  The row meets its CPU-fixed gate, and against the session wholly on the host the integers are equal and the offsets within
    1e-4 px"""
    lost, at, after, gate = M.ROWS[name]
    frames, poses, steps = M.row_frames(name, 1)
    ro = M.opts()
    s, cam, mir = fleet(), 1, Mirror(mref)

    def track(i):
        s.push([cam], frames[i:i + 1])
        out = s.keyframe_track([cam], steps[i:i + 1], **TRACK_KW)[0]
        want = mir.track(out, frames[i], steps[i], TRACK)
        assert out.tobytes() == want.tobytes(), (i, out["flags"], want["flags"])
        assert mir.same_map(s, cam) and _images(s, cam).tobytes() == mir.images.tobytes() and s.keyframe(cam).tobytes() == mir.key.tobytes(), i
        return out
    for i in range(at + 1):
        before_rec = track(i)
    entries, mstate = s.keyframe_map_info(cam)
    images = _images(s, cam)
    ok, hb = M.ref_origin_curr(mref, mir.state)
    slot, grid, start = M.ref_select(mref, mstate, entries, hb, ro.min_grid)
    rv = s.keyframe_revisit([cam], **M.opts_kw(ro))[0]
    assert s.last_keyframe_device_ms() > 0.0
    assert ok and (int(rv["slot"]), int(rv["grid"])) == (slot, grid) == (0, 64) and rv["start_px"].tobytes() == start.tobytes()
    assert rv["h_origin_before"].tobytes() == hb.tobytes() == before_rec["h_origin_curr"].tobytes()
    rec = eng.op_photo_align_robust(images[slot][None], frames[at:at + 1], start[None], levels=ro.levels, max_iterations=K.TRIALS)
    assert rv["rec"].tobytes() == rec.tobytes()
    want, attach = mir.revisit(hb, slot, grid, start, rec, ro)
    assert rv.tobytes() == want.tobytes(), (rv["flags"], want["flags"])
    assert attach and int(rv["flags"]) == _capi.RV_ATTACHED and int(rv["links"]) == 0
    assert s.keyframe(cam).tobytes() == images[slot].tobytes() == frames[0].tobytes()
    assert mir.same_map(s, cam) and _images(s, cam).tobytes() == images.tobytes()
    b, a = M.worst_px(rv["h_origin_before"], poses[at]), M.worst_px(rv["h_origin_curr"], poses[at])
    print(f"{name}, seed 1, device: corners of h_origin_curr at frame {at}: {b:.3e} px off the truth before the revisit, {a:.3e} px after (gate {gate:.3e})")
    assert a <= gate and (a < b if name == "closure-sub-pixel" else b >= M.BEFORE_RATIO * gate)
    nxt = [track(i) for i in after]
    assert nxt[0]["age"] == 1 and nxt[0]["keyframes"] == before_rec["keyframes"] + 1 and not nxt[0]["flags"] & _capi.KF_LOST
    assert int(mir.entries[int(mir.mstate["cur_slot"][0])]["links"]) == 2                # slot 0's links 0, one per re-key since
    recs, rrv, rafter, _ = M.ref_row(mref, name, 1)
    assert (recs["flags"][at], rrv["flags"], rrv["slot"], rrv["links"], rrv["grid"]) == (before_rec["flags"], rv["flags"], rv["slot"], rv["links"], rv["grid"])
    assert [int(r["flags"]) for r in nxt] == rafter["flags"].tolist()
    assert np.abs(rv["key_px"].astype(np.float64) - rrv["key_px"]).max() <= OFFSETS_VS_REFERENCE_PX
    assert np.abs(nxt[1]["key_px"].astype(np.float64) - rafter[1]["key_px"]).max() <= OFFSETS_VS_REFERENCE_PX


@pytest.mark.parametrize("name", list(M.ROWS))
def test_accuracy(fleet, name):
    """the row on four cameras at once, seeds 1, 2, 5, 11 (calls of n = 4, ids out of order): every camera attaches slot 0 and meets the CPU file's gate;
    closure-at-origin and recovery: "before" is at least 3 gates; closure-sub-pixel: "after" is below "before" for each seed"""
    lost, at, _, gate = M.ROWS[name]
    seqs = [M.row_frames(name, seed) for seed in U.SEEDS]
    ids = [2, 0, 3, 1]
    s = fleet()
    for i in range(at + 1):
        s.push(ids, np.stack([q[0][i] for q in seqs]))
        out = s.keyframe_track(ids, np.stack([q[2][i] for q in seqs]), **TRACK_KW)
    assert (out["flags"] == (134 if lost is not None else _capi.KF_REKEYED | _capi.KF_MAX_AGE)).all(), out["flags"]
    rv = s.keyframe_revisit(ids, **M.opts_kw(M.opts()))
    assert (rv["flags"] == _capi.RV_ATTACHED).all() and (rv["slot"] == 0).all() and (rv["links"] == 0).all(), (rv["flags"], rv["slot"])
    for j, seed in enumerate(U.SEEDS):
        pose = seqs[j][1][at]
        b, a = M.worst_px(rv[j]["h_origin_before"], pose), M.worst_px(rv[j]["h_origin_curr"], pose)
        print(f"{name}, seed {seed}, device: {b:.3e} px off the truth before the revisit, {a:.3e} px after (gate {gate:.3e})")
        assert rv[j]["h_origin_before"].tobytes() == out[j]["h_origin_curr"].tobytes() and a <= gate
        assert a < b if name == "closure-sub-pixel" else b >= M.BEFORE_RATIO * gate
        assert s.keyframe(ids[j]).tobytes() == seqs[j][0][0].tobytes()


def test_map_does_not_disturb_the_track(fleet):
    """two fleets, with and without a map, run the same 9 frames with max_age = 1: track records and get_keyframe are equal byte for byte at every frame"""
    seqs = [K.sequence("out-and-back", seed) for seed in (2, 11)]
    ids = [3, 1]
    a, b = fleet(), fleet(capacity=None)
    for i in range(9):
        recs = []
        for s in (a, b):
            s.push(ids, np.stack([q[0][i] for q in seqs]))
            recs.append(s.keyframe_track(ids, np.stack([q[2][i] for q in seqs]), **TRACK_KW))
        assert recs[0].tobytes() == recs[1].tobytes(), i
        assert (recs[0]["flags"] == (FIRST if i == 0 else _capi.KF_REKEYED | _capi.KF_MAX_AGE)).all()
        for c in ids:
            assert a.keyframe(c).tobytes() == b.keyframe(c).tobytes()
    with pytest.raises(_capi.HnetError) as ei:
        b.keyframe_map_info(1)
    assert ei.value.status == INVALID


@pytest.mark.parametrize("capacity", [2, 3])
def test_eviction(fleet, mref, capacity):
    """the 9 frames with max_age = 1 at capacities 2 (a ring of one slot) and 3: map_info and every stored image equal the mirror's after every frame,
    and slot 0 is frame 0 throughout"""
    frames, _, steps = K.sequence("out-and-back", 5)
    s, cam, mir = fleet(capacity=capacity), 2, Mirror(mref, capacity)
    for i in range(9):
        s.push([cam], frames[i:i + 1])
        out = s.keyframe_track([cam], steps[i:i + 1], **TRACK_KW)[0]
        assert out.tobytes() == mir.track(out, frames[i], steps[i], TRACK).tobytes(), i
        entries, mstate = s.keyframe_map_info(cam)
        assert len(entries) == capacity and entries.tobytes() == mir.entries.tobytes() and mstate.tobytes() == mir.mstate.tobytes(), (i, entries, mir.entries)
        imgs = _images(s, cam, capacity)
        assert imgs.tobytes() == mir.images.tobytes() and imgs[0].tobytes() == frames[0].tobytes(), i
        want_slot = 0 if i == 0 else 1 + (i - 1) % (capacity - 1)
        assert (int(mstate["cur_slot"][0]), int(mstate["cur_links"][0]), int(mstate["serial"][0])) == (want_slot, i, i + 1)
        assert imgs[want_slot].tobytes() == frames[i].tobytes() and (int(entries[0]["valid"]), int(entries[0]["links"]), int(entries[0]["serial"])) == (1, 0, 1)
    for other in (0, 1, 3):                                                  # the sessions no call listed hold nothing
        entries, mstate = s.keyframe_map_info(other)
        assert not entries.view(np.uint8).any() and not mstate.view(np.uint8).any() and not _images(s, other, capacity).any()


def _hygiene_fleets(fleet):
    """two identical fleets: session 2 never re-keyed, 0 three re-keys along a whole-pixel translation, 3 on the recovery path, 1 seven re-keys along the
    translation -> (fleets, the frame each session holds)"""
    tr, _, tr_steps = K.sequence("translation-32", 2)
    oab, _, oab_steps = K.sequence("out-and-back", 5)
    rec, _, rec_steps = M.row_frames("recovery", 1)
    plan = {2: (oab, oab_steps, 2, K.opts_kw(K.opts())), 0: (tr, tr_steps, 3, TRACK_KW), 3: (rec, rec_steps, 5, TRACK_KW), 1: (tr, tr_steps, 7, TRACK_KW)}
    fleets = (fleet(), fleet())
    for s in fleets:
        for cam, (frames, steps, last, kw) in plan.items():
            for i in range(last + 1):
                s.push([cam], frames[i:i + 1])
                out = s.keyframe_track([cam], steps[i:i + 1], **kw)
            assert out["keyframes"][0] == (1 if cam == 2 else last + 1)
    return fleets, plan


def _keyframe(s, cam):
    """the session's keyframe, or None when it holds none"""
    try:
        return s.keyframe(cam).tobytes()
    except _capi.HnetError as e:
        assert e.status == NOT_READY
        return None


def _snapshot(s, cam):
    """everything the keyframe layers hold of a session: (entries, map state, images, keyframe)"""
    entries, mstate = s.keyframe_map_info(cam)
    return entries.tobytes(), mstate.tobytes(), _images(s, cam).tobytes(), _keyframe(s, cam)


def test_slot_hygiene(fleet):
    """one call lists four sessions out of order, with min_grid 64 and max_closure_px 1e-3: session 2 has no candidate (it never re-keyed), 0 is attached
    to slot 0 (whole-pixel shifts close to 3e-5 px), 3 is rejected on the recovery path (its closure is 0.6 px) and 1 is attached to a ring slot (slot
    0, 28 px away, has 56 grid points inside).  Each record, map, keyframe and next track equals the same session revisited alone on a second fleet; a
    call that lists one session leaves the others' maps, images and keyframes as they are"""
    (a, b), plan = _hygiene_fleets(fleet)
    kw = M.opts_kw(M.opts(min_grid=64, max_closure_px=1e-3))
    order = [3, 1, 2, 0]
    keep = {c: _snapshot(a, c) for c in range(N_CAM)}
    one = a.keyframe_revisit([1], **kw)[0]
    for c in (0, 2, 3):
        assert _snapshot(a, c) == keep[c], c
    alone = {c: b.keyframe_revisit([c], **kw)[0] for c in (0, 1, 2, 3)}
    assert one.tobytes() == alone[1].tobytes()
    a2 = fleet()                                                             # a third fleet takes the call of four: fleet a has revisited session 1 already
    for cam, (frames, steps, last, tkw) in plan.items():
        for i in range(last + 1):
            a2.push([cam], frames[i:i + 1])
            a2.keyframe_track([cam], steps[i:i + 1], **tkw)
    out = a2.keyframe_revisit(order, **kw)
    got = {c: out[j] for j, c in enumerate(order)}
    for c in range(N_CAM):
        assert got[c].tobytes() == alone[c].tobytes(), (c, got[c]["flags"], alone[c]["flags"])
        assert _snapshot(a2, c) == _snapshot(b, c), c
    assert int(got[2]["flags"]) == _capi.RV_NO_CANDIDATE and int(got[2]["slot"]) == -1 and not got[2]["rec"].tobytes().strip(b"\0")
    assert got[2]["start_px"].view(np.uint32).tolist() == [0x7FC00000] * 8 and _snapshot(a2, 2) == keep[2]
    assert int(got[0]["flags"]) == _capi.RV_ATTACHED and (int(got[0]["slot"]), int(got[0]["links"]), int(got[0]["grid"])) == (0, 0, 64)
    assert int(got[3]["flags"]) == _capi.RV_CLOSURE_ABOVE_MAX and int(got[3]["slot"]) == 0 and _snapshot(a2, 3) == keep[3]
    assert np.abs(got[3]["rec"]["px"]["offsets_px"] - got[3]["start_px"]).max() > 0.1 and not got[3]["closure_px"].any()
    assert int(got[1]["flags"]) == _capi.RV_ATTACHED and (int(got[1]["slot"]), int(got[1]["links"]), int(got[1]["grid"])) == (2, 6, 64)
    tr = plan[1][0]
    assert a2.keyframe(0).tobytes() == tr[0].tobytes() and a2.keyframe(1).tobytes() == tr[6].tobytes() and a2.keyframe(2).tobytes() == plan[2][0][0].tobytes()
    assert a2.keyframe(3).tobytes() == plan[3][0][5].tobytes()
    # the states, by the next track of every session: the same frames once more (a GAP) on both fleets
    nxt = a2.keyframe_track(order, None, **TRACK_KW)
    for j, c in enumerate(order):
        assert nxt[j].tobytes() == b.keyframe_track([c], None, **TRACK_KW)[0].tobytes(), c
    assert nxt[1]["age"] == 1 and nxt[3]["age"] == 1 and nxt[0]["age"] == 1                 # attached sessions start a new age; 3 re-keyed at every frame anyway


def test_resets(fleet):
    """hnet_sessions_keyframe_reset and hnet_sessions_reset leave the session with no valid entry and a zero map state, other sessions as they are, and
    its next track is FIRST into slot 0"""
    frames, _, steps = K.sequence("out-and-back", 2)
    s, ids = fleet(), [0, 1, 2]
    for i in range(4):
        s.push(ids, np.stack([frames[i]] * 3))
        s.keyframe_track(ids, np.stack([steps[i]] * 3), **TRACK_KW)
    keep = _snapshot(s, 2)
    assert s.keyframe_map_info(0)[0]["valid"].tolist() == [1, 1, 1]
    s.keyframe_reset(0)
    s.reset(1)
    s.push([1], frames[5:6])
    for cam in (0, 1):
        entries, mstate = s.keyframe_map_info(cam)
        assert not entries.view(np.uint8).any() and not mstate.view(np.uint8).any()
        with pytest.raises(_capi.HnetError) as ei:
            s.keyframe_revisit([cam], **M.opts_kw(M.opts()))
        assert ei.value.status == NOT_READY
    assert _snapshot(s, 2) == keep
    out = s.keyframe_track([1, 0], None, **TRACK_KW)
    assert (out["flags"] == FIRST).all() and (out["keyframes"] == 1).all()
    for cam, frame in ((0, frames[3]), (1, frames[5])):
        entries, mstate = s.keyframe_map_info(cam)
        assert entries["valid"].tolist() == [1, 0, 0] and (int(entries[0]["links"]), int(entries[0]["serial"])) == (0, 1)
        assert entries[0]["h_origin_key"].tobytes() == np.eye(3).tobytes()
        assert (int(mstate["cur_slot"][0]), int(mstate["cur_links"][0]), int(mstate["cursor"][0]), int(mstate["serial"][0])) == (0, 0, 0, 1)
        assert s.map_keyframe(cam, 0).tobytes() == frame.tobytes() == s.keyframe(cam).tobytes()
    rv = s.keyframe_revisit([0, 1, 2], **M.opts_kw(M.opts()))
    assert rv["flags"].tolist() == [_capi.RV_NO_CANDIDATE, _capi.RV_NO_CANDIDATE, _capi.RV_ATTACHED] and _snapshot(s, 2)[0] == keep[0] and _snapshot(s, 2)[2] == keep[2]


def test_read_only(fleet):
    """two identical fleets with identical infers, one with tracks and revisits between them, the other without keyframes at all: means, covariances,
    sequence numbers, image counts, stamps and hnet_sessions_photo_align_robust's records on the consecutive pair are equal byte for byte; a rejected
    revisit leaves map_info, the images and get_keyframe untouched"""
    frames, _, steps = K.sequence("out-and-back", 5)
    a, b = fleet(), fleet(keyframes=False)
    ids = [1, 3]
    attached = 0
    for i in range(5):
        for s in (a, b):
            s.push(ids, np.stack([frames[i], frames[i + 1]]), t=[float(i), float(i)])
        a.keyframe_track(ids, np.stack([steps[i], steps[i + 1]]), **TRACK_KW)
        if i == 0:
            continue
        prior = np.stack([steps[i], steps[i + 1]]).astype(np.float64)
        ma, ca = a.infer(ids, prior)
        keep = {c: _snapshot(a, c) for c in ids}
        timing = a.last_timing()
        rej = a.keyframe_revisit(ids[::-1], **M.opts_kw(M.opts(max_closure_px=1e-6)))
        assert (rej["flags"] == _capi.RV_CLOSURE_ABOVE_MAX).all() and (rej["slot"] == 0).all(), (i, rej["flags"])     # (slot 0 has links 0, the held keyframe 1)
        for c in ids:
            assert _snapshot(a, c) == keep[c], (i, c)
        rv = a.keyframe_revisit(ids, **M.opts_kw(M.opts()))
        attached += int((rv["flags"] == _capi.RV_ATTACHED).sum())
        assert a.last_timing() == timing
        mb, cb = b.infer(ids, prior)
        assert ma.tobytes() == mb.tobytes() and ca.tobytes() == cb.tobytes()
        ra = a.photo_align_robust(ids, prior.astype(np.float32), levels=K.LEVELS, max_iterations=K.TRIALS)
        rb = b.photo_align_robust(ids, prior.astype(np.float32), levels=K.LEVELS, max_iterations=K.TRIALS)
        assert ra.tobytes() == rb.tobytes()
        for c in range(N_CAM):
            assert (a.seq(c), a.image_count(c), a.latest_time(c)) == (b.seq(c), b.image_count(c), b.latest_time(c))
            if c in ids:
                assert a.frame(c, 1).tobytes() == b.frame(c, 1).tobytes() and a.frame(c, 0).tobytes() == b.frame(c, 0).tobytes()
    assert attached >= 2


def test_errors_change_nothing(eng, fleet):
    """every refusal: enable before the keyframes, with a capacity of 1 or 9, twice, or when a session already holds a keyframe; a revisit before the
    map is enabled, with a repeated id, n > max_batch, a session with no image, one without a keyframe, one whose latest image no track saw, levels 0
    and 5, min_grid 0 and 65, min_overlap 1.5, negative limits, a null opts or out; map_info and get_map_keyframe out of range.  Each returns its code,
    writes nothing and changes nothing - the maps, keyframes and next records are those of a fleet that never saw the refused calls"""
    L = _capi.lib()
    frames, _, steps = K.sequence("out-and-back", 11)
    size = M.REVISIT.itemsize
    out = np.full(9 * size, 0xA5, np.uint8)
    keep = out.copy()

    def call(s, ids, o, outp=out.ctypes.data):
        ids = np.asarray(ids, np.int32)
        return L.hnet_sessions_keyframe_revisit(s._s, len(ids), ids.ctypes.data, C.addressof(o) if o is not None else None, outp)
    ok = M.opts()
    never, nomap, late, a, b = fleet(keyframes=False), fleet(capacity=None), fleet(capacity=None), fleet(), fleet()
    assert L.hnet_sessions_enable_keyframe_map(never._s, 3) == INVALID and L.hnet_sessions_enable_keyframe_map(None, 3) == INVALID
    assert L.hnet_sessions_enable_keyframe_map(nomap._s, 1) == INVALID and L.hnet_sessions_enable_keyframe_map(nomap._s, 9) == INVALID
    assert L.hnet_sessions_enable_keyframe_map(a._s, 3) == INVALID                                      # twice
    late.push([2], frames[:1])
    late.keyframe_track([2], None, **TRACK_KW)
    assert L.hnet_sessions_enable_keyframe_map(late._s, 3) == INVALID                                   # session 2 holds a keyframe already
    for s in (never, nomap, late):
        s.push([0], frames[:1])
        assert call(s, [0], ok) == INVALID
        assert L.hnet_sessions_keyframe_map_info(s._s, 0, out.ctypes.data, out.ctypes.data) == INVALID
        assert L.hnet_sessions_get_map_keyframe(s._s, 0, 0, out.ctypes.data) == INVALID
    for s in (a, b):
        for i in range(3):
            s.push([0, 1], frames[i:i + 2])
            s.keyframe_track([0, 1], steps[i:i + 2], **TRACK_KW)
        s.push([2], frames[:1])                                                                         # an image, no keyframe
        s.push([1], frames[4:5])                                                                        # an image its last track did not see
    snap = {c: _snapshot(a, c) for c in range(N_CAM)}
    assert call(a, [0, 0], ok) == INVALID and call(a, [4], ok) == INVALID and call(a, [-1], ok) == INVALID and call(a, [], ok) == INVALID
    assert call(a, [0, 1, 2, 3, 0, 1, 2, 3, 0], ok) == CAPACITY
    assert call(a, [0, 3], ok) == NOT_READY and call(a, [0, 2], ok) == NOT_READY and call(a, [0, 1], ok) == NOT_READY
    for bad in (dict(levels=0), dict(levels=5), dict(min_grid=0), dict(min_grid=65), dict(min_overlap=1.5), dict(min_overlap=-0.5), dict(max_mse=-1.0),
                dict(max_closure_px=-1.0), dict(max_closure_px=float("inf")), dict(huber_k=-1.0), dict(max_iterations=33)):
        assert call(a, [0], M.opts(**bad)) == INVALID, bad
    assert call(a, [0], ok, outp=None) == INVALID and call(a, [0], None) == INVALID
    assert L.hnet_sessions_keyframe_revisit(None, 1, None, None, None) == INVALID
    assert L.hnet_sessions_keyframe_map_info(a._s, 4, out.ctypes.data, out.ctypes.data) == INVALID
    assert L.hnet_sessions_keyframe_map_info(a._s, 0, None, out.ctypes.data) == INVALID
    assert L.hnet_sessions_get_map_keyframe(a._s, 0, 3, out.ctypes.data) == INVALID and L.hnet_sessions_get_map_keyframe(a._s, 0, -1, out.ctypes.data) == INVALID
    assert L.hnet_sessions_get_map_keyframe(a._s, 4, 0, out.ctypes.data) == INVALID and L.hnet_sessions_get_map_keyframe(a._s, 0, 0, None) == INVALID
    assert out.tobytes() == keep.tobytes()
    for c in range(N_CAM):
        assert _snapshot(a, c) == snap[c] == _snapshot(b, c), c
    ra, rb = a.keyframe_revisit([0], **M.opts_kw(ok)), b.keyframe_revisit([0], **M.opts_kw(ok))
    assert ra.tobytes() == rb.tobytes() and ra["flags"][0] == _capi.RV_ATTACHED
    ta, tb = a.keyframe_track([1, 0], None, **TRACK_KW), b.keyframe_track([1, 0], None, **TRACK_KW)
    assert ta.tobytes() == tb.tobytes() and ta["flags"][1] & _capi.KF_GAP and not ta["flags"][0] & _capi.KF_GAP
    assert a.keyframe_revisit([1], **M.opts_kw(ok)).tobytes() == b.keyframe_revisit([1], **M.opts_kw(ok)).tobytes()          # tracked now: no longer refused
