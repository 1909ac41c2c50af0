"""Recovering a lost camera inside the track (include/hnet.h hnet_sessions_keyframe_track_recover; include/hnet_keyframe_recover.h) on the CPU:
the layouts and defaults of the two structs; every outcome of the header's decide_deferred and finish on inputs of their own, against the existing decide
under both values of auto_rekey; the host restatement of the whole call (tests/cpp/keyframe_recover_ref.cpp) against two twins built from the existing
reference calls alone; the four kidnapped rows under auto_rekey = 1 and max_mse = 120 against the existing gates; and the core under AddressSanitizer +
UBSan (tests/cpp/keyframe_recover_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import keyframe_recover_util as KR
import keyframe_util as K
import photo_align_util as U
import photo_search_oriented_util as O
import photo_search_util as S
from cuahn_vio_amd import _capi

ROOT = U.ROOT


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return KR.build_ref(tmp_path_factory.mktemp("keyframe_recover_ref"))


@pytest.fixture(scope="module")
def tab(ref):
    return O.yaw_table(ref)


def test_layouts_and_defaults(ref):
    """the two structs are the track's and the oriented relocalise's side by side; the defaults are theirs, and max_mse stays 0"""
    assert _capi.KF_RECOVERED == 2048 and not _capi.KF_RECOVERED & (_capi.KF_LOST | 1023 | _capi.KF_ORIGIN_RESTARTED)
    assert KR.RECOVER.fields["track"][1] == 0 and KR.RECOVER.fields["reloc"][1] == K.TRACK.itemsize
    assert KR.RECOVER["track"] == K.TRACK and KR.RECOVER["reloc"] == O.ORELOC
    assert _capi.KeyframeRecoverOpts.track.offset == 0 and _capi.KeyframeRecoverOpts.reloc.offset == C.sizeof(_capi.KeyframeOpts)
    o = _capi.KeyframeRecoverOpts()
    C.memset(C.byref(o), 0xA5, C.sizeof(o))
    ref.keyframe_recover_ref_default_opts(C.byref(o))
    want_t, want_r = K.opts(max_iterations=o.track.align.base.max_iterations), S.reloc_opts(max_iterations=o.reloc.align.base.max_iterations)
    assert bytes(o.track) == bytes(want_t) and bytes(o.reloc) == bytes(want_r)
    assert o.track.max_mse == 0.0 and o.track.auto_rekey == 1 and o.track.levels == 3 and o.reloc.levels == 4
    z = KR.zero_reloc(ref)
    assert z["target"] == _capi.RL_TARGET_NONE
    z["target"] = 0
    assert not z.tobytes().strip(b"\0")


def _held_state():
    s = K.new_state()
    s["has_key"], s["age"], s["keyframes"] = 1, 2, 3
    s["key_px"][0] = np.array([3.0, -2.0, 3.5, -1.0, 2.0, -2.5, 3.0, -1.5], np.float32)
    s["h_origin_key"][0] = np.array([[1.0, 0.01, 12.0], [-0.01, 1.0, -7.0], [1e-5, -2e-5, 1.0]])
    return s


def _record(flags=0, mse=10.0, offsets=None, n_valid=60000):
    r = np.zeros(1, K.REC)
    r["px"]["flags"], r["px"]["mse"], r["px"]["n_valid"] = flags, mse, n_valid
    r["px"]["offsets_px"][0] = np.array([4.0, -1.0, 4.5, -0.5, 3.0, -2.0, 4.0, -1.0], np.float32) if offsets is None else offsets
    return r


START = np.array([3.5, -1.5, 4.0, -1.0, 2.5, -2.0, 3.5, -1.0], np.float32)
NAN8 = np.full(8, np.nan, np.float32)
LOST_CASES = {
    _capi.KF_NO_START: (NAN8, _record(flags=U.DEGENERATE)),
    _capi.KF_STOPPED: (START, _record(flags=U.SINGULAR)),
    _capi.KF_MSE_ABOVE_MAX: (START, _record(mse=400.0)),
    _capi.KF_NON_FINITE: (START, _record(offsets=NAN8)),
}
RL_OUTCOMES = (_capi.RL_RETRACKED, _capi.RL_ATTACHED, _capi.RL_NO_CANDIDATE, _capi.RL_STOPPED, _capi.RL_MSE_ABOVE_MAX, _capi.RL_NON_FINITE, _capi.RL_LOW_OVERLAP,
               _capi.RL_CLOSURE_ABOVE_MAX, _capi.RL_CHAIN)


@pytest.mark.parametrize("auto_rekey", [0, 1])
def test_not_lost_and_first(ref, auto_rekey):
    """a tracked frame (with and without a LOW_OVERLAP / MAX_AGE re-key) and a first frame: state, record and copy flag are decide's, nothing is active and
    the stash is zero"""
    for state, rec, kw in ((_held_state(), _record(), {}), (_held_state(), _record(n_valid=30000), {}), (_held_state(), _record(), dict(max_age=3)),
                           (K.new_state(), _record(), {})):
        o = K.opts(auto_rekey=auto_rekey, max_mse=KR.MAX_MSE, **kw)
        ns, out, stash, active, cp = KR.ref_decide(ref, state, START, rec, o, gap=True)
        ns1, out1, cp1 = K.ref_decide(ref, state, START, rec, o, gap=True)
        assert (ns.tobytes(), out.tobytes(), cp, active) == (ns1.tobytes(), out1.tobytes(), cp1, 0) and not stash.tobytes().strip(b"\0")
        assert not KR.ref_decide(ref, state, START, rec, o)[1]["flags"][0] & _capi.KF_LOST
    assert out["flags"][0] == _capi.KF_FIRST | _capi.KF_REKEYED


@pytest.mark.parametrize("auto_rekey", [0, 1])
@pytest.mark.parametrize("why", sorted(LOST_CASES))
def test_every_lost_outcome(ref, why, auto_rekey):
    """each LOST reason under each outcome of the relocalise: decide_deferred commits T0 and keeps T1; finish gives T0 | RECOVERED on the state the
    relocalise left, or T1 and its copy flag, byte for byte the existing decide's under auto_rekey = 0 and under the caller's"""
    start, rec = LOST_CASES[why]
    state = _held_state()
    o, o0 = K.opts(auto_rekey=auto_rekey, max_mse=KR.MAX_MSE), K.opts(auto_rekey=0, max_mse=KR.MAX_MSE)
    s0, t0, c0 = K.ref_decide(ref, state, start, rec, o0)
    s1, t1, c1 = K.ref_decide(ref, state, start, rec, o)
    assert t0["flags"][0] & _capi.KF_LOST == why and c0 == 0 and c1 == auto_rekey and bool(t1["flags"][0] & _capi.KF_REKEYED) == bool(auto_rekey)
    assert ref.keyframe_recover_ref_lost_of(int(t0["flags"][0])) == why
    ns, out, stash, active, cp = KR.ref_decide(ref, state, start, rec, o)
    assert (ns.tobytes(), out.tobytes(), cp, active) == (s0.tobytes(), t0.tobytes(), 0, 1)
    assert stash["state"].tobytes() == s1.tobytes() and stash["copy"][0] == c1 and stash["flags"][0] == t1["flags"][0]
    left = ns.copy()                                   # the state a relocalise leaves: another key_px, age 0
    left["key_px"][0] += 1.25
    left["age"] = 0
    for outcome in RL_OUTCOMES:
        fs, ft, c2 = KR.ref_finish(ref, outcome, stash, left, out)
        if outcome in (_capi.RL_RETRACKED, _capi.RL_ATTACHED):
            want = t0.copy()
            want["flags"] |= _capi.KF_RECOVERED
            assert (fs.tobytes(), ft.tobytes(), c2) == (left.tobytes(), want.tobytes(), 0), outcome
        else:
            assert (fs.tobytes(), ft.tobytes(), c2) == (s1.tobytes(), t1.tobytes(), c1), outcome


def _run_row(ref, tab, name, seed, auto_rekey=1):
    """the row on the host session with both twins checked at every call -> (records, outcomes, the session)"""
    r = KR.row(name, seed)
    ses = KR.RefRecoverSession(ref, KR.capacity(name))
    o = KR.recover_opts(KR.track_opts(name, auto_rekey), KR.reloc_opts(name))
    recs, whats = [], []
    for i, frame in enumerate(r["frames"]):
        before = ses.clone()
        out, what = ses.track_recover(frame, r["steps"][i], o, tab)
        KR.check_against_twins(ses, out, what, *KR.twins(before, frame, r["steps"][i], o, tab, lost=what != KR.NOT_LOST))
        recs.append(out)
        whats.append(what)
    return recs, whats, ses


@pytest.mark.parametrize("name", KR.ROWS)
def test_rows(ref, tab, name):
    """the four rows over seeds 1, 2, 5, 11 with auto_rekey = 1, max_mse = 120 and the default yaw table: the kidnapped frame is MSE_ABOVE_MAX | BRIDGED |
    RECOVERED and ends inside the row's existing gate where the plain track ends at least BEFORE_RATIO gates off, the constant frame of the map rows is
    lost and unrecovered and is the plain track's bridged re-key, the next frame is TRACKED; every call equals its twin byte for byte"""
    g = KR.gate(name)
    for seed in KR.SEEDS:
        r = KR.row(name, seed)
        recs, whats, _ = _run_row(ref, tab, name, seed)
        lost, nxt = recs[r["lost"]], recs[r["next"]]
        for i, rec in enumerate(recs):                 # the separation max_mse = 120 relies on
            mse = float(rec["track"]["rec"]["px"]["mse"])
            if i == (r["lost"] if r["constant"] is None else r["constant"]):
                assert mse > KR.LOST_ABOVE, (seed, i, mse)
            elif i == r["lost"]:                       # the far frame of a map row is measured against the constant keyframe: lost, whatever its mse
                assert whats[i] != KR.NOT_LOST
            elif i > 0:
                assert mse * 3 < KR.MAX_MSE and whats[i] == KR.NOT_LOST, (seed, i, mse)
        flags = int(lost["track"]["flags"])
        err = KR.row_error(name, lost, r["pose"])
        assert whats[r["lost"]] == KR.RECOVERED and flags & _capi.KF_RECOVERED and flags & _capi.KF_LOST and not flags & _capi.KF_REKEYED, (seed, flags)
        if name.endswith("_map"):
            c = recs[r["constant"]]
            assert whats[r["constant"]] == KR.UNRECOVERED and c["track"]["flags"] & _capi.KF_LOST and c["track"]["flags"] & _capi.KF_REKEYED
            assert c["track"]["flags"] & _capi.KF_BRIDGED and not c["track"]["flags"] & _capi.KF_RECOVERED
            assert c["reloc"]["rv"]["flags"] == _capi.RL_NO_CANDIDATE and c["reloc"]["n_found"] == 0 and c["reloc"]["n_searched"] >= 1
            t = S.ref_thumbnail(ref, r["frames"][r["constant"]])
            assert O.ref_search(ref, S.ref_thumbnail(ref, r["frames"][0]), t, S.search_opts(), tab)[0]["base"]["flags"][0] == _capi.PS_NO_TEXTURE
            assert lost["reloc"]["rv"]["flags"] == _capi.RL_ATTACHED and lost["reloc"]["target"] >= 0
        else:
            assert flags == _capi.KF_MSE_ABOVE_MAX | _capi.KF_BRIDGED | _capi.KF_RECOVERED, (seed, flags)
            assert lost["reloc"]["rv"]["flags"] == _capi.RL_RETRACKED and lost["reloc"]["target"] == _capi.RL_TARGET_HELD
        # the contrast: the same frames through the plain track with the same options
        plain = S.RefRelocSession(ref, KR.capacity(name))
        to = KR.track_opts(name)
        before = [plain.track(r["frames"][i], r["steps"][i], to) for i in range(r["lost"] + 1)][-1]
        e_plain = KR.plain_error(name, before, r["pose"])
        print(f"{name}, seed {seed}: lost flags {flags}, entry {lost['reloc']['search']['hyp']}, target {lost['reloc']['target']}; {err:.4f} px after the call "
              f"(gate {g:.4f}), {e_plain:.2f} px through the plain track; track mse {float(lost['track']['rec']['px']['mse']):.1f}")
        assert before["flags"] & _capi.KF_REKEYED and before["flags"] & _capi.KF_LOST
        assert err <= g and e_plain >= S.BEFORE_RATIO * g
        assert whats[r["next"]] == KR.NOT_LOST and not nxt["track"]["flags"] & (_capi.KF_LOST | _capi.KF_RECOVERED)


@pytest.mark.parametrize("name", ["kidnapped", "kidnapped_map"])
def test_rows_without_auto_rekey(ref, tab, name):
    """the same calls under auto_rekey = 0 equal their twins too: an unrecovered frame keeps the keyframe, a recovered one is the same record"""
    recs, whats, _ = _run_row(ref, tab, name, 5, auto_rekey=0)
    r = KR.row(name, 5)
    if r["constant"] is None:
        assert whats[r["lost"]] == KR.RECOVERED
    else:                                              # without a re-key the keyframe is still frame 0 and the far frame, 2 px from it, simply tracks
        c = recs[r["constant"]]["track"]
        assert whats[r["constant"]] == KR.UNRECOVERED and not c["flags"] & _capi.KF_REKEYED


def test_keyframe_recover_check_under_asan_ubsan(tmp_path):
    """the header's outcomes and one whole row under AddressSanitizer + UBSan: a stand-alone program; nothing loaded into python is sanitized"""
    exe = str(tmp_path / "keyframe_recover_check_san.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *U.HOST_FLAGS,
                    os.path.join(ROOT, "tests", "cpp", "keyframe_recover_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "keyframe_recover_check: ok" in r.stdout
