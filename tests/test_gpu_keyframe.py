"""Tracking each camera against a held keyframe on the device (include/hnet.h hnet_sessions_keyframe_track; csrc/kernels_keyframe.hip): the
pinned identity with hnet_op_photo_align_robust and the host header, drift on an out-and-back path, slot hygiene, the re-key against the host reference,
read-only for everything the sessions had before, and the refusals.  levels = 3, 6 trials; sessions objects of 4 cameras on a context of max_batch 8."""
import ctypes as C

import numpy as np
import pytest

import keyframe_util as K
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, CAPACITY = 1, 4, 5
N_CAM = 4


@pytest.fixture(scope="module")
def kref(tmp_path_factory):
    return K.build_ref(tmp_path_factory.mktemp("keyframe_ref_gpu"))


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

    def make(keyframes=True):
        s = HnetSessions(eng, N_CAM)
        if keyframes:
            s.enable_keyframes()
        made.append(s)
        return s
    yield make
    for s in made:
        s.close()


def test_pinned_identity(eng, fleet, kref):
    """every frame of the 9-frame out-and-back sequence (max_age 3, so that the path re-keys): rec equals hnet_op_photo_align_robust(keyframe, curr,
    start_px) called afterwards with the same options, byte for byte, the keyframe downloaded before the track; start_px equals the host header's compose
    of the step and the state's key_px (difference 0); the whole record equals the host header's decide on that record, byte for byte"""
    frames, _, steps = K.sequence("out-and-back", 1)
    o = K.opts(max_age=3)
    kw = K.opts_kw(o)
    s, cam = fleet(), 1
    state = K.new_state()
    rekeys = 0
    for i in range(len(frames)):
        s.push([cam], frames[i:i + 1])
        if i == 0:
            with pytest.raises(_capi.HnetError) as ei:
                s.keyframe(cam)
            assert ei.value.status == NOT_READY
            key = None
        else:
            key = s.keyframe(cam)
        out = s.keyframe_track([cam], steps[i:i + 1], **kw)
        assert s.last_keyframe_device_ms() > 0.0
        if i == 0:
            start, rec = np.zeros(8, np.float32), np.zeros(1, K.REC)
        else:
            start = K.ref_compose(kref, steps[i], state["key_px"][0])
            assert start is not None and out["start_px"][0].tobytes() == start.tobytes(), (i, out["start_px"][0], start)
            rec = eng.op_photo_align_robust(key[None], frames[i:i + 1], start[None], levels=o.levels, max_iterations=K.TRIALS)
            assert out["rec"].tobytes() == rec.tobytes(), i
        state, want, copy = K.ref_decide(kref, state, start, rec, o)
        assert out.tobytes() == want.tobytes(), (i, out[0], want[0])
        assert s.keyframe(cam).tobytes() == (frames[i] if copy else key).tobytes(), i
        rekeys += copy
    assert rekeys == 3 and out["keyframes"][0] == 3 and not (out["flags"][0] & _capi.KF_LOST)


def test_drift(fleet):
    """out-and-back with steps of the truth plus 0.3 px pseudo-noise: at frame 8, the keyframe's pose, key_px is within the CPU-fixed gate of zero, while
    the plain sum of the same steps is at least 3 gates off (asserted on the host reference in tests/test_keyframe_cpu.py; restated here on the input)"""
    overlap, gate, _ = K.ROWS["out-and-back"]
    s = fleet()
    seeds = (2, 5, 11)
    seqs = [K.sequence("out-and-back", seed) for seed in seeds]
    ids = [3, 0, 2]
    for i in range(9):
        s.push(ids, np.stack([q[0][i] for q in seqs]))
        out = s.keyframe_track(ids, np.stack([q[2][i] for q in seqs]), **K.opts_kw(K.opts(rekey_overlap=overlap)))
        assert (out["flags"] == (_capi.KF_FIRST | _capi.KF_REKEYED if i == 0 else 0)).all() and (out["age"] == i).all(), (i, out["flags"])
    for j, seed in enumerate(seeds):
        off, drift = float(np.abs(out["key_px"][j]).max()), float(np.abs(K.chained_sum(seqs[j][2], 8)).max())
        print(f"seed {seed}: frame 8: key_px {off:.3e} px off zero; chained sum of the steps {drift:.4f} px off")
        assert off <= gate and drift >= K.DRIFT_RATIO * gate and out["keyframes"][j] == 1


def test_slot_hygiene(fleet):
    """n = 1, ids = [2, 0] out of order, and one call in which session 3 is FIRST, 0 is TRACKED, 1 is LOST (its current frame is constant: SINGULAR, an
    ordinary input) and re-keyed and 2 re-keys on low overlap: each session's record and its keyframe afterwards equal those of the same session tracked
    alone (n = 1 calls on a second fleet), and unlisted sessions keep their keyframes and their state (their next records are the second fleet's)"""
    oab, _, oab_steps = K.sequence("out-and-back", 1)
    tr, tr_poses, _ = K.sequence("translation-32", 2)
    const = np.full((224, 320), 93, np.uint8)
    kw = K.opts_kw(K.opts(rekey_overlap=0.9))
    first = {0: oab[0], 1: oab[2], 2: tr[0], 3: oab[4]}
    second = {0: oab[1], 1: const, 2: tr[8]}
    step2 = {0: oab_steps[1], 1: np.zeros(8, np.float32), 2: K.relative(tr_poses[0], tr_poses[8]).astype(np.float32), 3: np.zeros(8, np.float32)}
    third = {0: oab[2], 1: oab[3], 2: tr[9], 3: oab[3]}
    a, b = fleet(), fleet()
    for s in (a, b):
        s.push([0, 1, 2], np.stack([first[i] for i in (0, 1, 2)]))
    ra = {}
    out = a.keyframe_track([2, 0], None, **kw)
    ra[2], ra[0] = out[0], out[1]
    ra[1] = a.keyframe_track([1], None, **kw)[0]
    rb = {i: b.keyframe_track([i], None, **kw)[0] for i in (0, 1, 2)}
    for i in (0, 1, 2):
        assert ra[i].tobytes() == rb[i].tobytes() and ra[i]["flags"] == _capi.KF_FIRST | _capi.KF_REKEYED
        assert a.keyframe(i).tobytes() == first[i].tobytes()
    for s in (a, b):
        s.push([0, 1, 2, 3], np.stack([second[0], second[1], second[2], first[3]]))
    order = [3, 1, 0, 2]
    out = a.keyframe_track(order, np.stack([step2[i] for i in order]), **kw)
    alone = {i: b.keyframe_track([i], step2[i][None], **kw)[0] for i in (0, 1, 2, 3)}
    for j, i in enumerate(order):
        assert out[j].tobytes() == alone[i].tobytes(), (i, out[j]["flags"], alone[i]["flags"])
        assert a.keyframe(i).tobytes() == b.keyframe(i).tobytes()
    got = {i: int(out[j]["flags"]) for j, i in enumerate(order)}
    assert got[3] == _capi.KF_FIRST | _capi.KF_REKEYED and got[0] == 0
    assert got[1] == _capi.KF_STOPPED | _capi.KF_REKEYED | _capi.KF_BRIDGED and out[1]["rec"]["px"]["flags"] & 2
    assert got[2] == _capi.KF_LOW_OVERLAP | _capi.KF_REKEYED
    assert a.keyframe(0).tobytes() == first[0].tobytes() and a.keyframe(1).tobytes() == const.tobytes()
    assert a.keyframe(2).tobytes() == tr[8].tobytes() and a.keyframe(3).tobytes() == first[3].tobytes()
    # a call that lists session 1 alone leaves 0, 2, 3 as they are: keyframes now, states by their next records
    for s in (a, b):
        s.push([0, 1, 2, 3], np.stack([third[i] for i in range(4)]))
    keep = {i: a.keyframe(i) for i in (0, 2, 3)}
    one = a.keyframe_track([1], None, **kw)[0]
    assert one.tobytes() == b.keyframe_track([1], None, **kw)[0].tobytes() and one["keyframes"] >= 2
    for i in (0, 2, 3):
        assert a.keyframe(i).tobytes() == keep[i].tobytes()
    rest = a.keyframe_track([0, 3, 2], None, **kw)
    for j, i in enumerate((0, 3, 2)):
        assert rest[j].tobytes() == b.keyframe_track([i], None, **kw)[0].tobytes(), i
    assert rest[0]["age"] == 2 and rest[1]["age"] == 1 and rest[2]["age"] == 1 and rest[2]["keyframes"] == 2


def test_rekey_matches_reference(fleet, kref):
    """the 32 px translation at rekey_overlap 0.9: REKEYED appears at the host reference's frame; after it the keyframe is that tick's current frame;
    keyframes and age equal the reference's at every frame; h_origin_curr is within the gate of the truth over the whole path"""
    overlap, gate_key, gate_origin = K.ROWS["translation-32"]
    frames, poses, steps = K.sequence("translation-32", 1)
    ref = K.ref_row(kref, "translation-32", 1)
    s, cam = fleet(), 2
    kw = K.opts_kw(K.opts(rekey_overlap=overlap))
    recs = []
    for i in range(len(frames)):
        s.push([cam], frames[i:i + 1])
        r = s.keyframe_track([cam], steps[i:i + 1], **kw)[0]
        recs.append(r)
        assert (int(r["flags"]), int(r["age"]), int(r["keyframes"])) == (int(ref[i]["flags"]), int(ref[i]["age"]), int(ref[i]["keyframes"])), i
        if r["flags"] & _capi.KF_REKEYED:
            assert s.keyframe(cam).tobytes() == s.frame(cam, 1).tobytes() == frames[i].tobytes()
    recs = np.stack(recs)
    assert [i for i in range(1, len(recs)) if recs[i]["flags"] & _capi.KF_REKEYED] == [8]
    wk, wo = K.worst_key_px(recs, poses), K.worst_origin_px(recs, poses)
    print(f"translation-32, device: key_px {wk:.3e} px, corners of h_origin_curr {wo:.3e} px off the truth at the worst frame")
    assert wk <= gate_key and wo <= gate_origin


def test_read_only(fleet):
    """two identical fleets with identical infers, one with keyframe tracks between them, the other without keyframes at all: means, covariances,
    sequence numbers, image counts and hnet_sessions_photo_align_robust's records on the consecutive pair are equal byte for byte; hnet_sessions_reset
    followed by a track gives FIRST, and so does hnet_sessions_keyframe_reset"""
    frames, _, steps = K.sequence("out-and-back", 5)
    a, b = fleet(), fleet(keyframes=False)
    ids = [1, 3]
    kw = K.opts_kw(K.opts())
    for i in range(4):
        for s in (a, b):
            s.push(ids, np.stack([frames[i], frames[i + 1]]), t=[float(i), float(i)])
        timing = a.last_timing()
        tr = a.keyframe_track(ids, np.stack([steps[i], steps[i + 1]]), **kw)
        assert a.last_timing() == timing
        assert (tr["flags"] == (_capi.KF_FIRST | _capi.KF_REKEYED if i == 0 else 0)).all(), (i, tr["flags"])
        if i == 0:
            continue
        prior = np.stack([steps[i], steps[i + 1]]).astype(np.float64)
        ma, ca = a.infer(ids, prior)
        again = a.keyframe_track(ids[::-1], None, **kw)                   # (the same frames once more: no new image since the previous track, which is a GAP)
        assert (again["flags"] == _capi.KF_GAP).all() and (again["age"] == 2 * i).all()
        mb, cb = b.infer(ids, prior)
        assert ma.tobytes() == mb.tobytes() and ca.tobytes() == cb.tobytes()
        ra = a.photo_align_robust(ids, prior.astype(np.float32), levels=K.LEVELS, max_iterations=K.TRIALS)
        rb = b.photo_align_robust(ids, prior.astype(np.float32), levels=K.LEVELS, max_iterations=K.TRIALS)
        assert ra.tobytes() == rb.tobytes()
        for c in range(N_CAM):
            assert (a.seq(c), a.image_count(c), a.latest_time(c)) == (b.seq(c), b.image_count(c), b.latest_time(c))
    a.reset(1)
    a.keyframe_reset(3)
    with pytest.raises(_capi.HnetError) as ei:
        a.keyframe(1)
    assert ei.value.status == NOT_READY
    with pytest.raises(_capi.HnetError) as ei:
        a.keyframe_track([1], None, **kw)                                 # (hnet_sessions_reset dropped its images too)
    assert ei.value.status == NOT_READY
    a.push([1], frames[7:8])
    out = a.keyframe_track([1, 3], None, **kw)
    assert (out["flags"] == _capi.KF_FIRST | _capi.KF_REKEYED).all() and (out["keyframes"] == 1).all()
    assert a.keyframe(1).tobytes() == frames[7].tobytes() and a.keyframe(3).tobytes() == frames[4].tobytes()


def test_errors_change_nothing(eng, fleet):
    """track before enable, a second enable, a repeated id, n > max_batch, a session with no image, levels 0 and 5, rekey_overlap 1.5, a negative max_mse,
    auto_rekey 2, a null out: each returns its code, writes nothing and changes nothing - the next records and the keyframes are those of a fleet that
    never saw the refused calls"""
    L = _capi.lib()
    frames, _, steps = K.sequence("out-and-back", 11)
    never, a, b = fleet(keyframes=False), fleet(), fleet()
    size = K.TRACK.itemsize
    out = np.full(9 * size, 0xA5, np.uint8)
    keep = out.copy()

    def call(s, ids, o, outp=out.ctypes.data):
        ids = np.asarray(ids, np.int32)
        return L.hnet_sessions_keyframe_track(s._s, len(ids), ids.ctypes.data, None, C.addressof(o) if o is not None else None, outp)
    ok = K.opts()
    never.push([0], frames[:1])
    assert call(never, [0], ok) == INVALID and L.hnet_sessions_keyframe_reset(never._s, 0) == INVALID
    assert L.hnet_sessions_get_keyframe(never._s, 0, out.ctypes.data) == INVALID and L.hnet_sessions_last_keyframe_device_ms(never._s) == 0.0
    for s in (a, b):
        s.push([0, 1], frames[:2])
        s.keyframe_track([0, 1], None, **K.opts_kw(ok))
        s.push([0, 1], frames[1:3])
    assert L.hnet_sessions_enable_keyframes(a._s) == INVALID
    assert call(a, [0, 0], ok) == INVALID and call(a, [4], ok) == INVALID and call(a, [], ok) == INVALID
    assert call(a, [0, 1, 2, 3, 0, 1, 2, 3, 0], ok) == CAPACITY
    assert call(a, [0, 2], ok) == NOT_READY
    for bad in (dict(levels=0), dict(levels=5), dict(rekey_overlap=1.5), dict(max_mse=-1.0), dict(auto_rekey=2), dict(max_age=-1), dict(huber_k=-1.0),
                dict(max_iterations=33)):
        assert call(a, [0, 1], K.opts(**bad)) == INVALID, bad
    assert call(a, [0, 1], ok, outp=None) == INVALID and call(a, [0, 1], None) == INVALID
    assert L.hnet_sessions_keyframe_track(None, 1, None, None, None, None) == INVALID
    assert out.tobytes() == keep.tobytes()
    for i in (0, 1):
        assert a.keyframe(i).tobytes() == b.keyframe(i).tobytes() == frames[i].tobytes()
    ra, rb = a.keyframe_track([0, 1], steps[1:3], **K.opts_kw(ok)), b.keyframe_track([0, 1], steps[1:3], **K.opts_kw(ok))
    assert ra.tobytes() == rb.tobytes() and (ra["flags"] == 0).all() and (ra["age"] == 1).all()
