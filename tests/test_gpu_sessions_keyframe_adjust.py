"""hnet_sessions_keyframe_adjust on the device (include/hnet.h; csrc/capi_keyframe_adjust.hip): maps built by tracking frames of one canvas
along a path adjust like hnet_op_keyframe_adjust on the images and entries read back from the session; with apply the map holds the record's matrices,
the state follows entry cur_slot and the next keyframe is chained from the adjusted matrix; sessions whose jobs fill a round exactly and straddle one
get the records they get alone; unlisted sessions and a call without apply keep every byte; every refusal returns its code and changes nothing; and a
sessions object that enabled the layer but never called it, or calls it without apply, tracks and revisits as one without it.  Sessions objects of 4
cameras with maps of capacity 8 on a context of max_batch 8; the tracks re-key at every frame (keyframe_adjust_util.TRACK_KW)."""
import ctypes as C

import numpy as np
import pytest

import keyframe_adjust_util as A
import keyframe_map_util as M
import keyframe_util as K
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, CAPACITY = 1, 4, 5
N_CAM, CAP = 4, 8
ADJUSTED = _capi.ADJ_ADJUSTED
KW = dict(A.TEXTURE_OPTS)


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("keyframe_adjust_ref_sessions"))


@pytest.fixture(scope="module")
def mref(tmp_path_factory):
    return M.build_ref(tmp_path_factory.mktemp("keyframe_map_ref_adjust"))


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

    def make(adjust=True, keymap=True):
        s = HnetSessions(eng, N_CAM)
        s.enable_keyframes()
        if keymap:
            s.enable_keyframe_map(CAP)
        if adjust:
            s.enable_keyframe_adjust()
        made.append(s)
        return s
    yield make
    for s in made:
        s.close()


def _track(s, cams, seqs, begin, end):
    """frames begin .. end - 1 of each camera's sequence, the steps the truth -> the last call's records"""
    out = None
    for i in range(begin, end):
        s.push(cams, np.stack([q[0][i] for q in seqs]))
        out = s.keyframe_track(cams, np.stack([q[2][i] for q in seqs]), **A.TRACK_KW)
    return out


def _map(s, cam):
    entries, mstate = s.keyframe_map_info(cam)
    return np.stack([s.map_keyframe(cam, j) for j in range(CAP)]), entries, mstate


def _keyframe(s, cam):
    try:
        return s.keyframe(cam).tobytes()
    except _capi.HnetError as e:                                               # (a session without a keyframe)
        assert e.status == NOT_READY
        return None


def _snapshot(s, cam):
    """everything the sessions and the keyframe layers hold of a session"""
    images, entries, mstate = _map(s, cam)
    frame = s.frame(cam, 1).tobytes() if s.image_count(cam) else None
    return images.tobytes(), entries.tobytes(), mstate.tobytes(), _keyframe(s, cam), frame, s.image_count(cam)


def test_end_to_end(eng, aref, mref, fleet):
    """a fleet of 4 tracked round the loop, two of them revisited at its end, all adjusted with apply: each record equals the operator's on the map read
    back before the call; the map afterwards holds the record's matrices with valid, links, serial, the map state and the images unchanged; and the
    next track's h_origin_curr is chained from entry cur_slot's ADJUSTED matrix, so the state followed it"""
    s = fleet()
    cams = [0, 1, 2, 3]
    seqs = [A.path_frames(seed, closed=True) for seed in (2, 4, 5, 7)]
    _track(s, cams, seqs, 0, 7)
    rv = s.keyframe_revisit([0, 1], **M.opts_kw(M.opts()))
    print("revisit flags", rv["flags"], "slots", rv["slot"], "closure", np.abs(rv["closure_px"]).max(axis=1))
    assert (rv["flags"] == _capi.RV_ATTACHED).any()
    before = {c: _map(s, c) for c in cams}
    keys = {c: _keyframe(s, c) for c in cams}
    ids = [2, 0, 3, 1]
    rec, er = s.keyframe_adjust(ids, want_edge_records=True, apply=1, **KW)
    assert s.last_keyframe_device_ms() > 0.0
    moved_state = 0
    for k, c in enumerate(ids):
        images, ent, ms = before[c]
        assert int(ent["valid"].sum()) == 7
        orec, oer = eng.op_keyframe_adjust(images, ent, want_edge_records=True, **KW)
        r = rec[k]
        print("camera", c, "flags", int(r["flags"]), "jobs", int(r["n_jobs"]), "edges", int(r["n_edges"]), "trials", int(r["trials"]), "cost0 %.4g cost %.4g" %
              (r["cost0"], r["cost"]), "worst |delta| %.3f px" % np.abs(r["delta_px"]).max(), "cur_slot", int(ms[0]["cur_slot"]))
        assert r.tobytes() == orec[0].tobytes() and er[k].tobytes() == oer.tobytes(), c
        assert int(r["flags"]) & ADJUSTED and int(r["anchor"]) == 0 and int(r["n_jobs"]) > 8
        images2, ent2, ms2 = _map(s, c)
        assert ent2["h_origin_key"].tobytes() == r["h_origin_key"].tobytes() and ent2["h_origin_key"].tobytes() != ent["h_origin_key"].tobytes()
        for f in ("valid", "links", "serial", "pad"):
            assert ent2[f].tobytes() == ent[f].tobytes(), (c, f)
        assert images2.tobytes() == images.tobytes() and ms2.tobytes() == ms.tobytes() and _keyframe(s, c) == keys[c]
    # the next frame: every session re-keys, and its new keyframe is chained from the adjusted matrix of the entry it hung on
    after = {c: _map(s, c) for c in cams}
    s.push(cams, np.stack([q[0][1] for q in seqs]))
    tr = s.keyframe_track(cams, np.stack([q[2][1] for q in seqs]), **A.TRACK_KW)
    for k, c in enumerate(cams):
        _, ent, ms = after[c]
        cur = int(ms[0]["cur_slot"])
        assert int(tr[k]["flags"]) & _capi.KF_REKEYED and not int(tr[k]["flags"]) & _capi.KF_LOST and cur >= 0
        state = K.new_state()
        state["has_key"], state["key_px"], state["h_origin_key"] = 1, tr[k]["key_px"], ent[cur]["h_origin_key"]
        ok, h = M.ref_origin_curr(mref, state)
        assert ok and np.asarray(h).tobytes() == tr[k]["h_origin_curr"].tobytes(), c
        old = K.new_state()
        old["has_key"], old["key_px"], old["h_origin_key"] = 1, tr[k]["key_px"], before[c][1][cur]["h_origin_key"]
        moved_state += np.asarray(M.ref_origin_curr(mref, old)[1]).tobytes() != tr[k]["h_origin_curr"].tobytes()
        _, ent3, ms3 = _map(s, c)
        new = int(ms3[0]["cur_slot"])
        assert ent3[new]["h_origin_key"].tobytes() == tr[k]["h_origin_curr"].tobytes() and int(ent3[new]["links"]) == int(ent[cur]["links"]) + 1
    assert moved_state >= 2                                                    # (the sessions that were not re-attached to the anchor hung on a moved entry)


def _three_maps(s):
    """camera 0: 4 frames of the loop (6 jobs), camera 1: 3 frames (3 jobs), camera 2: the diagonal (3 pairs, 2 jobs); camera 3: nothing"""
    _track(s, [0], [A.path_frames(2)], 0, 4)
    _track(s, [1], [A.path_frames(4)], 0, 3)
    _track(s, [2], [A.path_frames(5, A.DIAGONAL_PATH)], 0, 3)


def test_rounds_and_independence(eng, aref, fleet):
    """job totals of exactly 8 (one full round) and 9 (the second session straddles the round boundary): every record equals the one the session gets
    alone; the same session as slot 0 and as slot 2 of 3, twice, in equal bytes; a session without entries says ADJ_FEW_ENTRIES"""
    s = fleet()
    _three_maps(s)
    alone = {c: s.keyframe_adjust([c], want_edge_records=True, **KW) for c in range(N_CAM)}
    jobs = {c: int(alone[c][0][0]["n_jobs"]) for c in range(N_CAM)}
    print("jobs", jobs, "pairs", {c: int(alone[c][0][0]["n_pairs"]) for c in range(N_CAM)}, "flags", {c: int(alone[c][0][0]["flags"]) for c in range(N_CAM)})
    assert jobs == {0: 6, 1: 3, 2: 2, 3: 0} and int(alone[2][0][0]["n_pairs"]) == 3
    for c in (0, 1, 2):
        images, ent, _ = _map(s, c)
        t = A.ref_pairs(aref, ent, 32)[0]
        assert int(t["count"]) == jobs[c]                                      # the header's pairs on the entries read back
        orec, oer = eng.op_keyframe_adjust(images, ent, want_edge_records=True, **KW)
        assert alone[c][0].tobytes() == orec.tobytes() and alone[c][1][0].tobytes() == oer.tobytes(), c
        assert A.bytes_equal(alone[c][0], A.ref_adjust_with(aref, ent, oer[:jobs[c]], A.opts(aref, **KW))[0])
    want = np.zeros(1, A.REC)
    want["flags"], want["anchor"], want["lambda"] = _capi.ADJ_FEW_ENTRIES, -1, 1e-3
    assert alone[3][0].tobytes() == want.tobytes() and not alone[3][1].view(np.uint8).any()
    for ids in ([0, 2], [0, 1], [1, 0], [2, 0, 1], [0, 1, 2, 3], [1, 3, 0], [0, 2], [0, 1]):
        rec, er = s.keyframe_adjust(ids, want_edge_records=True, **KW)
        assert sum(int(r["n_jobs"]) for r in rec) == sum(jobs[c] for c in ids)
        for k, c in enumerate(ids):
            assert rec[k].tobytes() == alone[c][0][0].tobytes() and er[k].tobytes() == alone[c][1][0].tobytes(), (ids, c)
    got = []
    for ids in ([1, 0, 2], [0, 2, 1], [1, 0, 2], [0, 2, 1]):                    # camera 1 as slot 0 and as slot 2 of 3, twice
        rec = s.keyframe_adjust(ids, **KW)
        got.append(rec[ids.index(1)].tobytes())
    assert all(g == alone[1][0][0].tobytes() for g in got)


def test_left_alone(fleet):
    """unlisted sessions keep every byte under an applied adjustment of the others; without apply the listed ones do too"""
    s = fleet()
    _three_maps(s)
    s.push([3], A.path_frames(7)[0][:1])
    snap = {c: _snapshot(s, c) for c in range(N_CAM)}
    rec = s.keyframe_adjust([0, 1, 2, 3], apply=0, **KW)
    assert (rec["flags"][:3] & ADJUSTED).all()
    for c in range(N_CAM):
        assert _snapshot(s, c) == snap[c], c
    rec1 = s.keyframe_adjust([1, 3], apply=1, **KW)
    assert rec1[0].tobytes() == rec[1].tobytes() and rec1[1].tobytes() == rec[3].tobytes()
    for c in (0, 2, 3):
        assert _snapshot(s, c) == snap[c], c
    now = _snapshot(s, 1)
    assert now[1] != snap[1][1] and now[0] == snap[1][0] and now[2:] == snap[1][2:]                          # the entries moved, and nothing else


def test_untouched_paths(fleet):
    """a sessions object with the layer enabled and never called, and one that adjusts without apply between the calls, return track and revisit
    records byte for byte equal to one without the layer"""
    plain, enabled, used = fleet(adjust=False), fleet(), fleet()
    seqs = [A.path_frames(seed, closed=True) for seed in (4, 5)]
    ids = [1, 3]
    attached = 0
    for i in range(7):
        recs = []
        for s in (plain, enabled, used):
            s.push(ids, np.stack([q[0][i] for q in seqs]))
            recs.append(s.keyframe_track(ids, np.stack([q[2][i] for q in seqs]), **A.TRACK_KW))
        assert recs[0].tobytes() == recs[1].tobytes() == recs[2].tobytes(), i
        snap = {c: _snapshot(used, c) for c in ids}
        used.keyframe_adjust(ids, apply=0, **KW)
        used.keyframe_adjust(ids[::-1], want_edge_records=True, weighting=_capi.ADJ_WEIGHT_UNIT, **KW)
        for c in ids:
            assert _snapshot(used, c) == snap[c], (i, c)
        if i >= 5:
            rv = [s.keyframe_revisit(ids, **M.opts_kw(M.opts())) for s in (plain, enabled, used)]
            assert rv[0].tobytes() == rv[1].tobytes() == rv[2].tobytes(), i
            attached += int((rv[0]["flags"] == _capi.RV_ATTACHED).sum())
    assert attached >= 1
    for c in ids:
        assert _snapshot(plain, c) == _snapshot(enabled, c) == _snapshot(used, c)


def test_refusals_change_nothing(eng, fleet):
    """every refusal returns its code, writes nothing into the output buffers and leaves states, entries and images as they were"""
    L = _capi.lib()
    never, nomap, a = fleet(adjust=False), fleet(adjust=False, keymap=False), fleet()
    rec, er = np.full(9 * A.REC.itemsize, 0xA5, np.uint8), np.full(9 * 28 * A.ROBUST.itemsize, 0xA5, np.uint8)
    good = _capi.keyframe_adjust_opts(apply=1, **KW)

    def call(s, ids, o=good, recp=rec, erp=er):
        ids = np.asarray(ids, np.int32)
        p = lambda x: None if x is None else x.ctypes.data                     # noqa: E731
        return L.hnet_sessions_keyframe_adjust(s._s if s is not None else None, len(ids), ids.ctypes.data, C.addressof(o) if o is not None else None, p(recp), p(erp))
    # the enable: before the map, twice
    assert L.hnet_sessions_enable_keyframe_adjust(None) == INVALID and L.hnet_sessions_enable_keyframe_adjust(nomap._s) == INVALID
    assert L.hnet_sessions_enable_keyframe_adjust(a._s) == INVALID
    _three_maps(a)
    snap = {c: _snapshot(a, c) for c in range(N_CAM)}
    assert call(never, [0]) == INVALID and call(nomap, [0]) == INVALID and call(None, [0]) == INVALID        # before the enable
    assert call(a, [0, 0]) == INVALID and call(a, [4]) == INVALID and call(a, [-1]) == INVALID and call(a, []) == INVALID
    assert call(a, [0, 1, 2, 3, 0, 1, 2, 3, 0]) == CAPACITY
    assert call(a, [0], o=None) == INVALID and call(a, [0], recp=None) == INVALID
    for k, v in (("levels", 0), ("levels", 5), ("min_grid", 0), ("min_grid", 65), ("min_overlap", 1.5), ("max_mse", -1.0), ("max_closure_px", np.nan),
                 ("weighting", 2), ("max_trials", 0), ("max_trials", 65), ("mse_floor", 0.0), ("lambda0", 0.0), ("lambda0", 1e101), ("eps_px", -1.0),
                 ("max_shift_px", np.inf), ("apply", 2), ("huber_k", -1.0), ("max_iterations", 33)):
        assert call(a, [0, 1], o=_capi.keyframe_adjust_opts(**{k: v})) == INVALID, (k, v)
    assert (rec == 0xA5).all() and (er == 0xA5).all()
    for c in range(N_CAM):
        assert _snapshot(a, c) == snap[c], c
    # and what they were variations of is good; a session without entries is no refusal; the edge records are optional
    assert call(a, [0, 1, 2, 3]) == 0 and call(a, [3], erp=None) == 0 and not (rec == 0xA5).all()
