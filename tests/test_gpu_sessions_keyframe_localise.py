"""hnet_sessions_keyframe_localise on the device (include/hnet.h; csrc/capi_keyframe_localise.hip, kernels_keyframe_localise.hip): a fleet of 4
on keyframe_util.sequence("out-and-back") with max_age = 1 and capacity 8, localised at frame 8 - each record against the operator call on the map read back
and against the host header with the session's states, apply byte for byte, the next track, unlisted sessions and apply = 0; a three-frame flight on the wide
canvas that the revisit cannot serve; order and slot independence; three fleets (never enabled, enabled, enabled and used) with equal track and revisit
records; the refusals.  Main model prior-3, N = 16, max_batch 8."""
import numpy as np
import pytest

import keyframe_localise_util as KL
import keyframe_map_util as KM
import keyframe_util as K
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
SEEDS = (1, 2, 5, 11)
TRACK = dict(max_age=1, levels=3, max_iterations=6)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return KL.build_rule_ref(tmp_path_factory.mktemp("keyframe_localise_ref_sessions"))


OPEN = []          # every sessions object a test made: closed after each test, pass or fail, so that none outlives the module's engine


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=8)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _close_sessions():
    yield
    while OPEN:
        OPEN.pop().close()


def _fleet(eng, enable, frames=9, between=None):
    """4 sessions on out-and-back (seeds 1, 2, 5, 11), tracked over `frames` frames -> (sessions, the track records per frame); between(s, f): called after
    the track of frame f"""
    from cuahn_vio_amd.homography_net import HnetSessions
    seqs = [K.sequence("out-and-back", seed) for seed in SEEDS]
    s = HnetSessions(eng, 4)
    OPEN.append(s)
    s.enable_keyframes()
    s.enable_keyframe_map(8)
    if enable:
        s.enable_keyframe_localise()
    ids, recs = np.arange(4, dtype=np.int32), []
    for f in range(frames):
        s.push(ids, np.stack([q[0][f] for q in seqs]))
        recs.append(s.keyframe_track(ids, np.stack([q[2][f] for q in seqs]), **TRACK))
        if between:
            between(s, f)
    return s, recs, seqs


def _state(track, ent, ms):
    """the session's state as the store holds it: the last track's key_px, age and keyframes and, by 7ad's invariant, the h_origin_key of the entry of cur_slot"""
    st = np.zeros(1, K.STATE)
    st["has_key"], st["age"], st["keyframes"], st["key_px"] = 1, track["age"], track["keyframes"], track["key_px"]
    if track["flags"] & _capi.KF_REKEYED:          # (the record's key_px is the measurement against the OLD keyframe; the new state's is zero)
        st["age"], st["key_px"] = 0, 0.0
    assert ms["cur_slot"][0] >= 0
    st["h_origin_key"] = ent[int(ms["cur_slot"][0])]["h_origin_key"]
    return st


def _maps(s):
    return [s.keyframe_map_info(i) for i in range(4)]


def test_fleet_localised_at_frame_8(eng, lib):
    """four sessions localised at frame 8 in the order 2, 0, 3, 1: rec, used_mask, cover, flags, h_origin_curr and correction_px equal the operator call on the
    map read back with the ineligible entries invalidated; the whole record equals the host header with the session's states on the device's record; apply = 0
    keeps every byte of every map; with apply on sessions 3 and 1 the entries and map state read back equal the header's byte for byte, sessions 0 and 2 keep
    every byte, and the next track's h_origin_curr lies within 0.01 px of the chain it should continue (the localised one where applied)"""
    s, recs, seqs = _fleet(eng, True)
    last = recs[-1]
    before = _maps(s)
    images = [np.stack([s.map_keyframe(i, j) for j in range(8)]) for i in range(4)]
    order = np.array([2, 0, 3, 1], np.int32)
    out = s.keyframe_localise(order)
    assert s.last_keyframe_device_ms() > 0.0
    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(before, _maps(s))), "apply = 0 keeps every byte"
    o = KL.loc_opts()
    for r, i in zip(out, order):
        ent, ms = before[i]
        st = _state(last[i], ent, ms)
        used = KL.ref_eligible_mask(lib, ms, ent)
        assert r["used_mask"] == used and used and r["links_before"] == ms["cur_links"][0]
        assert np.abs(K.corners(r["h_origin_before"]) - K.corners(last[i]["h_origin_curr"])).max() < 1e-9
        # the operator call on the map read back: the eligible entries, the same view, the session's current frame
        elig = ent.copy()
        elig["valid"] = [(used >> j) & 1 for j in range(8)]
        op = eng.op_keyframe_localise(images[i], elig, r["h_origin_before"], seqs[i][0][8])[0]
        assert op["rec"].tobytes() == r["rec"].tobytes() and op["used_mask"] == used and op["cover"] == r["cover"] and op["flags"] == r["flags"]
        assert op["h_origin_curr"].tobytes() == r["h_origin_curr"].tobytes() and op["correction_px"].tobytes() == r["correction_px"].tobytes()
        # the host header with the session's states on the device's alignment record
        _, want, _, _, _ = KL.ref_decide(lib, st, ms, ent, used, int(round(float(r["cover"]) * 71680)), r["h_origin_before"], r["rec"], o)
        assert r.tobytes() == want[0].tobytes()
        err_b, err_a = np.abs(K.corners(r["h_origin_before"]) - seqs[i][1][8]).max(), np.abs(K.corners(r["h_origin_curr"]) - seqs[i][1][8]).max()
        print(f"session {i}: flags {r['flags']}, cover {r['cover']:.3f}, used {used:#x}, links {r['links_before']} -> {r['links']}, pose error {err_b:.3f} -> {err_a:.4f} px")
        # the floor is the twice-resampled imagery (7q: 0.08 px, 7ad: 0.10 - 0.21 px)
        assert r["flags"] == _capi.LOC_LOCALISED and err_a < 0.25 and r["links"] <= r["links_before"]
    # apply on two sessions: the states follow the header byte for byte, the others keep every byte, the next track continues from the corrected chain
    listed = np.array([3, 1], np.int32)
    got = s.keyframe_localise(listed, apply=1)
    after = _maps(s)
    for r, i in zip(got, listed):
        ent, ms = before[i]
        st = _state(last[i], ent, ms)
        loc, want, ns, nm, ne = KL.ref_decide(lib, st, ms, ent, int(r["used_mask"]), int(round(float(r["cover"]) * 71680)), r["h_origin_before"], r["rec"], KL.loc_opts(apply=1))
        assert loc == 1 and r.tobytes() == want[0].tobytes()
        assert after[i][0].tobytes() == ne.tobytes() and after[i][1].tobytes() == nm.tobytes()
        assert after[i][1]["cur_links"][0] == r["links"] and after[i][0][int(ms["cur_slot"][0])]["h_origin_key"].tobytes() == ns[0]["h_origin_key"].tobytes()
    for i in (0, 2):
        assert after[i][0].tobytes() == before[i][0].tobytes() and after[i][1].tobytes() == before[i][1].tobytes()
    ids = np.arange(4, dtype=np.int32)
    s.push(ids, np.stack([q[0][8] for q in seqs]))
    nxt = s.keyframe_track(ids, np.zeros((4, 8), np.float32), **TRACK)
    by = {int(i): r for r, i in zip(got, listed)}
    for i in range(4):
        want_h = by[i]["h_origin_curr"] if i in by else last[i]["h_origin_curr"]
        d = np.abs(K.corners(nxt[i]["h_origin_curr"]) - K.corners(want_h)).max()
        print(f"session {i}: the next track's h_origin_curr lies {d:.2e} px from {'the localised' if i in by else 'its own'} chain")
        assert d < 0.01
    s.close()


def test_order_and_slot_independence(eng):
    """a session gets the same bytes alone, first, last and in any order"""
    s, _, _ = _fleet(eng, True)
    full = s.keyframe_localise([0, 1, 2, 3])
    for ids in ([3], [3, 1], [2, 0, 3, 1], [1, 2]):
        got = s.keyframe_localise(ids)
        for r, i in zip(got, ids):
            assert r.tobytes() == full[i].tobytes(), (ids, i)
    s.close()


def test_three_fleets_track_and_revisit_alike(eng):
    """never enabled, enabled, and enabled and used (apply = 0) between the calls: equal track records at every frame and equal revisit records at the end"""
    runs = []
    for enable, between in ((False, None), (True, None), (True, lambda s, f: f >= 3 and s.keyframe_localise([f % 4, (f + 2) % 4]))):
        s, recs, _ = _fleet(eng, enable, between=between)
        rv = s.keyframe_revisit([0, 1, 2, 3], max_iterations=6)
        runs.append((np.stack(recs).tobytes(), rv.tobytes(), [m[0].tobytes() + m[1].tobytes() for m in _maps(s)]))
        s.close()
    assert runs[0] == runs[1] == runs[2]


def test_three_frame_flight_on_the_wide_canvas(eng):
    """frame 0 at (-200, 0), frame 1 at (+200, 0) (LOST and bridged on its exact step), frame 2 at (0, 0): the revisit has NO_CANDIDATE (every grid count is
    below 32), the localise is LOCALISED with a cover between 0.6 and 0.9 and states the camera's pose"""
    from cuahn_vio_amd.homography_net import HnetSessions
    cv = KL.wide_canvas(1)
    poses = [np.tile([200.0, 0.0], 4), np.tile([-200.0, 0.0], 4), np.zeros(8)]
    s = HnetSessions(eng, 2)
    OPEN.append(s)
    s.enable_keyframes()
    s.enable_keyframe_map(8)
    s.enable_keyframe_localise()
    for f, p in enumerate(poses):
        s.push([1], KL.render(cv, p)[None])
        step = np.zeros(8) if f == 0 else K.relative(poses[f - 1], p)
        t = s.keyframe_track([1], step[None].astype(np.float32), levels=3, max_iterations=6)
        print(f"frame {f}: track flags {t[0]['flags']:#x}, overlap {t[0]['overlap']:.3f}, keyframes {t[0]['keyframes']}")
    ent, ms = s.keyframe_map_info(1)
    print("entries valid", ent["valid"], "links", ent["links"], "map state", ms)
    true_pose = K.relative(poses[0], poses[2])                                 # against frame 0, the origin
    rv = s.keyframe_revisit([1], max_iterations=6)
    assert rv[0]["flags"] == _capi.RV_NO_CANDIDATE
    r = s.keyframe_localise([1], apply=1)[0]
    err_b, err_a = np.abs(K.corners(r["h_origin_before"]) - true_pose).max(), np.abs(K.corners(r["h_origin_curr"]) - true_pose).max()
    print(f"localise: flags {r['flags']}, cover {r['cover']:.3f}, overlap {r['overlap']:.3f}, used {r['used_mask']:#x}, links {r['links_before']} -> {r['links']}, "
          f"pose error {err_b:.4f} -> {err_a:.4f} px")
    assert r["flags"] == _capi.LOC_LOCALISED and 0.6 < r["cover"] < 0.9 and bin(int(r["used_mask"])).count("1") == 2
    assert err_a < 0.25
    ent2, ms2 = s.keyframe_map_info(1)
    assert ms2["cur_links"][0] == r["links"] and ent2[int(ms2["cur_slot"][0])]["links"] == r["links"]
    s.close()


def test_refusals_change_nothing(eng):
    """a call before the enable, a second enable, refused options, a repeated or out-of-range id and a session without a tracked frame return their codes and leave
    every map as it was"""
    from cuahn_vio_amd.homography_net import HnetSessions
    s, _, seqs = _fleet(eng, False, frames=4)

    def refused(status, f):
        with pytest.raises(_capi.HnetError) as ei:
            f()
        assert ei.value.status == status
    refused(INVALID, lambda: s.keyframe_localise([0]))
    s.enable_keyframe_localise()
    refused(INVALID, lambda: s.enable_keyframe_localise())
    before = [m[0].tobytes() + m[1].tobytes() for m in _maps(s)]
    for kw in (dict(levels=0), dict(levels=5), dict(mode=3), dict(min_cover=1.5), dict(min_overlap=-0.1), dict(max_mse=-1.0), dict(max_shift_px=float("nan")), dict(apply=2),
               dict(huber_k=-1.0), dict(max_iterations=33)):
        refused(INVALID, lambda: s.keyframe_localise([0, 1], apply=1, **{k: v for k, v in kw.items()}) if "apply" not in kw else s.keyframe_localise([0, 1], **kw))
    refused(INVALID, lambda: s.keyframe_localise([0, 0], apply=1))
    refused(INVALID, lambda: s.keyframe_localise([4], apply=1))
    s.push([2], seqs[2][0][4][None])                                          # session 2's latest image is not the one its last track saw
    refused(NOT_READY, lambda: s.keyframe_localise([1, 2], apply=1))
    assert [m[0].tobytes() + m[1].tobytes() for m in _maps(s)] == before
    s.close()
    fresh = HnetSessions(eng, 2)
    OPEN.append(fresh)
    refused(INVALID, lambda: fresh.enable_keyframe_localise())                 # before the map
    fresh.close()
