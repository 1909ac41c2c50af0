"""The keyframe layers on hostile steps, on the host references (tests/cpp/keyframe_ref.cpp, keyframe_map_ref.cpp, photo_search_ref.cpp,
photo_search_oriented_ref.cpp), no GPU: the sequences of tests/keyframe_hostile.py run through the public shape of the calls (a step per
track, nothing hand-built), every flag word, the map's validity and state words and the relocalise's answer against that module's constants, every
h_origin_curr finite, and every byte of every output record written.  The GPU file asserts the same constants of the device.

"Every byte written": each record of a session is also produced by the header's decide on the state before the call with the output filled with 0xA5
(keyframe_util.ref_decide, keyframe_map_util.ref_decide), or by the same call on a copy of the session with the output filled with 0x5A (relocalise);
the two must agree byte for byte, which they cannot where a byte keeps its fill.

KF_NON_FINITE, RV_NON_FINITE, RL_NON_FINITE and RV_CHAIN: no input through the calls was found that reaches them, and the hand-built records of
tests/test_keyframe_cpu.py and tests/test_keyframe_map_cpu.py stay their only cover.  The three NON_FINITE flags need a non-finite offset in the record
of an alignment whose start was finite and which did not stop SINGULAR, DEGENERATE or FEW_PIXELS.  Tried on the host reference, as the second track of
a session (seed 5, auto_rekey = 0): steps with 1e15, 1e20, 1e30, 1e37, 3e38, FLT_MAX and -FLT_MAX in each single entry and in the entry sets (0, 1),
(0, 2), (4, 5), (0 .. 3), (0, 1, 6, 7) - 91 steps; and (0, 1) = 1e30, 3e38, FLT_MAX and the true step under lambda0 = 1e-300 and 1e100, eps_px = 0,
gain0 = 1e300, bias0 = 1e300, huber_k = 1e-300, min_valid = 1, and 32 trials with lambda0 = 1e-300 and min_valid = 1.  Every step either fails to
compose (NO_START, tested first) or gives a start on which level 0 stops (STOPPED, tested before NON_FINITE); gain0 and bias0 of 1e300 stop SINGULAR with
finite offsets.  An accepted trial has a finite cost over at least min_valid pixels inside the image, which bounds its offsets.  RV_CHAIN needs an entry
whose h_origin_key makes the product with H(offsets) degenerate while the alignment against that entry's image passed min_overlap: the entries a track
stores have passed chain() themselves, and the far ones (after a bridged 1e6 or 1e12 step) are never candidates (no grid point in view)."""
import ctypes as C

import numpy as np
import pytest

import keyframe_hostile as H
import keyframe_map_util as M
import keyframe_util as K
import photo_align_util as U
import photo_search_oriented_util as O
import photo_search_util as S
from cuahn_vio_amd import _capi


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    """one library: photo_search_oriented_ref.cpp includes the references of all the layers below it"""
    return O.build_ref(tmp_path_factory.mktemp("keyframe_hostile_ref"))


@pytest.fixture(scope="module")
def ran():
    """every case of this file runs once: case -> what it returned"""
    return {}


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _checked_track(ses, lib):
    """ses.track that also restates the record with the header's decide into a 0xA5-filled record"""
    def track(frame, step, o):
        before = ses.state.copy()
        out = ses.track(frame, step, o)
        ns, want, _ = K.ref_decide(lib, before, out["start_px"], out["rec"], o)
        assert want[0].tobytes() == out.tobytes() and ns.tobytes() == ses.state.tobytes(), "a byte of the track record keeps its fill"
        assert np.isfinite(out["h_origin_curr"]).all() and np.isfinite(ses.state["h_origin_key"]).all()
        return out
    return track


def _checked_revisit(ses, lib):
    def revisit(frame, o):
        state, mstate = ses.state.copy(), ses.mstate.copy()
        out = ses.revisit(frame, o)
        ns, nm, want, _ = M.ref_decide(lib, state, mstate, ses.entries, int(out["slot"]), int(out["grid"]), out["start_px"], out["h_origin_before"], out["rec"], o)
        assert want[0].tobytes() == out.tobytes() and ns.tobytes() == ses.state.tobytes() and nm.tobytes() == ses.mstate.tobytes(), "a byte keeps its fill"
        assert np.isfinite(out["h_origin_curr"]).all() and np.isfinite(out["h_origin_before"]).all()
        return out
    return revisit


def _track_case(lib, ran, seed, name, auto_rekey):
    key = ("track", seed, name, auto_rekey)
    if key not in ran:
        ran[key] = H.run_track(seed, name, auto_rekey, _checked_track(K.RefSession(lib), lib))
    return ran[key]


def _map_case(lib, ran, seed, name, auto_rekey):
    """-> (track records, revisit records, [(valid, map state)] after each of the last four calls)"""
    key = ("map", seed, name, auto_rekey)
    if key not in ran:
        ses, snaps = M.RefMapSession(lib), []

        def after(i):
            if H.map_snapshots(i) is not None:
                snaps.append((tuple(ses.entries["valid"].tolist()), tuple(int(ses.mstate[f][0]) for f in ("cur_slot", "cur_links", "cursor", "serial"))))
        ran[key] = H.run_map(seed, name, auto_rekey, _checked_track(ses, lib), _checked_revisit(ses, lib), after) + (snaps,)
    return ran[key]


def _copy_of(ses, lib):
    twin = O.RefSession(lib, ses.capacity)
    twin.state, twin.key, twin.mstate, twin.entries, twin.images = ses.state.copy(), ses.key.copy(), ses.mstate.copy(), ses.entries.copy(), ses.images.copy()
    return twin


def _relocalise_filled(ses, kind, frame, o, tab, fill):
    """the relocalise of `kind` on the session into a record filled with `fill`"""
    c = np.ascontiguousarray(frame, np.uint8).reshape(224, 320)
    out = np.zeros(1, S.RELOC if kind == "plain" else O.ORELOC)
    out.view(np.uint8)[:] = fill
    head = (_p(ses.state), _p(ses.key), _p(ses.mstate), _p(ses.entries), _p(ses.images), int(ses.capacity), _p(c), C.byref(o))
    if kind == "plain":
        ses.lib.photo_search_ref_relocalise(*head, None, _p(out))
    else:
        ses.lib.photo_search_oriented_ref_relocalise(*head, _p(tab), len(tab), None, _p(out))
    return out[0]


def _reloc_case(lib, ran, seed, kind):
    """-> (track records of frames 0 .. 3, the relocalise's record, frame 4's, the session afterwards)"""
    key = ("reloc", seed, kind)
    if key not in ran:
        ses = O.RefSession(lib, M.CAPACITY)
        tab = np.ascontiguousarray(O.yaw_table(lib)[H.YAW13])
        assert len(tab) == 13

        def relocalise(frame, o):
            twin = _copy_of(ses, lib)
            assert np.abs(ses.state["key_px"]).min() > 0.99e12                # poisoned: far outside the image
            out = ses.relocalise(frame, o) if kind == "plain" else ses.relocalise_oriented(frame, o, tab)
            again = _relocalise_filled(twin, kind, frame, o, tab, 0x5A)
            assert out.tobytes() == again.tobytes() and twin.snapshot() == ses.snapshot(), "a byte of the relocalise record keeps its fill"
            return out
        ran[key] = H.run_reloc(seed, _checked_track(ses, lib), relocalise) + (ses,)
    return ran[key]


@pytest.mark.parametrize("seed,name,auto_rekey", H.TRACK_CASES)
def test_track(lib, ran, seed, name, auto_rekey):
    """(a): the five flag words; a step that cannot be composed leaves the quiet-NaN start, a DEGENERATE record and, as the bridge, the previous key_px;
    a far finite step leaves its composed start as key_px; the keyframes count the re-key"""
    recs = _track_case(lib, ran, seed, name, auto_rekey)
    assert tuple(int(r["flags"]) for r in recs) == H.track_flags(seed, name, auto_rekey)
    hostile, before = recs[H.TRACK_AT], recs[H.TRACK_AT - 1]
    if name in H.NO_COMPOSE:
        assert K.ref_compose(lib, H.STEPS[name], before["key_px"]) is None
        assert hostile["start_px"].view(np.uint32).tolist() == [H.QNAN] * 8 and hostile["key_px"].tobytes() == before["key_px"].tobytes()
        assert hostile["rec"]["px"]["flags"] & U.DEGENERATE
    else:
        start = K.ref_compose(lib, H.STEPS[name], before["key_px"])
        assert start is not None and hostile["start_px"].tobytes() == start.tobytes() == hostile["key_px"].tobytes()
        assert np.abs(start).min() > 0.99 * float(name)
    assert [int(r["keyframes"]) for r in recs] == ([1, 1, 2, 2, 2] if auto_rekey else [1] * 5)


def test_stuck_session(lib):
    """auto_rekey = 0 after the 1e13 step: three further frames each answer NO_START | ORIGIN_RESTARTED and change nothing of the state but the age;
    a reset ends it: the next track is FIRST"""
    ses = M.RefMapSession(lib)
    states = []

    def track(frame, step, o):
        out = _checked_track(ses, lib)(frame, step, o)
        states.append((ses.state.copy(), ses.key.copy(), ses.entries.copy(), ses.mstate.copy()))
        return out
    recs, further = H.run_stuck(track)
    assert tuple(int(r["flags"]) for r in recs) == H.track_flags(H.STUCK_SEED, H.STUCK_STEP, 0)
    assert tuple(int(r["flags"]) for r in further) == H.STUCK_FLAGS
    for k, (r, (st, key, entries, mstate)) in enumerate(zip(further, states[H.TRACK_FRAMES:])):
        st0, key0, entries0, mstate0 = states[H.TRACK_FRAMES - 1]
        assert int(st["age"][0]) == H.STUCK_FURTHER[k] and st["key_px"].tobytes() == st0["key_px"].tobytes() and st["h_origin_key"].tobytes() == np.eye(3).tobytes()
        assert key.tobytes() == key0.tobytes() and entries.tobytes() == entries0.tobytes() and mstate.tobytes() == mstate0.tobytes()
        assert r["h_origin_curr"].tobytes() == np.eye(3).tobytes() and r["key_px"].tobytes() == st0["key_px"].tobytes() and not entries["valid"].any()
    ses.reset()
    frames, _, steps = K.sequence("out-and-back", H.STUCK_SEED)
    assert int(ses.track(frames[8], steps[8], H.track_opts(0))["flags"]) == H.FIRST


@pytest.mark.parametrize("seed,name,auto_rekey", H.MAP_CASES)
def test_map(lib, ran, seed, name, auto_rekey):
    """(b): the six track flag words, the two revisits' (flags, slot, links, grid), and the entries' valid and the map state after each of the last
    four calls; a revisit without a candidate aligned nothing"""
    recs, rvs, snaps = _map_case(lib, ran, seed, name, auto_rekey)
    want = H.MAP_EXPECT[name, auto_rekey]
    assert tuple(int(r["flags"]) for r in recs) == H.map_flags(seed, name, auto_rekey)
    assert tuple((int(r["flags"]), int(r["slot"]), int(r["links"]), int(r["grid"])) for r in rvs) == want["rv"]
    assert tuple(s[0] for s in snaps) == want["valid"] and tuple(s[1] for s in snaps) == want["mstate"], snaps
    for r in rvs:
        if r["flags"] == H.NO_CANDIDATE:
            assert r["start_px"].view(np.uint32).tolist() == [H.QNAN] * 8 and not r["rec"].tobytes().strip(b"\0")


@pytest.mark.parametrize("seed,kind", H.RELOC_CASES)
def test_relocalise_from_a_poisoned_session(lib, ran, seed, kind):
    """(c): the session whose key_px a 1e12 step left far outside the image.  The plain and the oriented relocalise both recover it: the held keyframe
    is searched and FOUND, the alignment from the searched start passes, RETRACKED replaces key_px (within the kidnapped rows' gate of the truth), and
    the next track with the true step is an ordinary tracked frame of the same keyframe"""
    recs, rl, nxt, ses = _reloc_case(lib, ran, seed, kind)
    frames, poses, _ = K.sequence("out-and-back", seed)
    assert tuple(int(r["flags"]) for r in recs) == H.RELOC_TRACKS[seed]
    assert (int(rl["rv"]["flags"]), int(rl["target"]), int(rl["n_searched"]), int(rl["n_found"])) == H.RELOC_ANSWER
    assert int(nxt["flags"]) == H.RELOC_NEXT and int(nxt["age"]) == H.RELOC_AT + 1 and int(nxt["keyframes"]) == 1
    assert np.isfinite(rl["rv"]["h_origin_curr"]).all() and np.isfinite(rl["rv"]["h_origin_before"]).all()
    e_rl, e_nxt = S.worst_px(rl["rv"]["key_px"], poses[H.RELOC_AT]), S.worst_px(nxt["key_px"], poses[H.RELOC_AT + 1])
    print(f"poisoned, seed {seed}, {kind}: key_px {e_rl:.4f} px off the truth after the relocalise, {e_nxt:.4f} px after the next track (gate {S.GATE_KIDNAPPED:.4f})")
    assert e_rl <= S.GATE_KIDNAPPED and e_nxt <= S.GATE_KIDNAPPED
    assert ses.state["key_px"][0].tobytes() == nxt["key_px"].tobytes() and ses.key.tobytes() == frames[0].tobytes()


def test_reached_flags(lib, ran):
    """the union of the flags the cases of this file reach holds every defensive branch the hostile steps are there for, and none of the four flags
    the module's docstring names"""
    kf = rv = rl = 0
    for case in H.TRACK_CASES:
        for r in _track_case(lib, ran, *case):
            kf |= int(r["flags"])
    for case in H.MAP_CASES:
        recs, rvs, _ = _map_case(lib, ran, *case)
        for r in recs:
            kf |= int(r["flags"])
        for r in rvs:
            rv |= int(r["flags"])
    for case in H.RELOC_CASES:
        recs, r, nxt, _ = _reloc_case(lib, ran, *case)
        rl |= int(r["rv"]["flags"])
    want = _capi.KF_NO_START | _capi.KF_STOPPED | _capi.KF_BRIDGED | _capi.KF_ORIGIN_RESTARTED | _capi.KF_REKEYED
    assert kf & want == want, kf
    assert rv == _capi.RV_NO_CANDIDATE | _capi.RV_ATTACHED and rl == _capi.RL_RETRACKED, (rv, rl)
    assert not kf & _capi.KF_NON_FINITE
