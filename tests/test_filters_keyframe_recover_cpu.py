"""CPU: recovering a lost camera inside the in-step keyframe track on the host (include/hnet_keyframe_measure_recover.h; include/hnet.h
hnet_filters_set_keyframe_recover) through tests/cpp/filters_keyframe_recover_ref.cpp: the layout of the new record, every reason of
usable_recover on an input of its own and in the header's order, next_prev_ok_recover, measure_recover against hnet_kfm::measure and on a RETRACKED
record, the twin property of hnet_ekf::iterated_update_keyframe_recovered - byte for byte iterated_update_keyframe_measured under a null recover option,
byte for byte RefRecoverSession.track_recover called by hand with recovery on - over 7u's four rows, the rows' table, and the stand-alone program
tests/cpp/filters_keyframe_recover_check.cpp under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filters_keyframe_recover_util as FR
import filters_keyframe_util as FK
import keyframe_recover_util as KR
import keyframe_util as KU
import photo_align_util as U
import photo_robust_util as R
import photo_search_oriented_util as O
import photo_search_util as S
import test_filters_keyframe_cpu as tk
import test_filters_photo_gate_cpu as tg
from cuahn_vio_amd import _capi, synth

ROOT = U.ROOT
LOST_BITS = (_capi.KF_NO_START, _capi.KF_STOPPED, _capi.KF_MSE_ABOVE_MAX, _capi.KF_NON_FINITE)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return FR.build_ref(tmp_path_factory.mktemp("filters_keyframe_recover_ref"))


@pytest.fixture(scope="module")
def tab(lib):
    return O.yaw_table(lib)


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    """two level-0 records of the host robust reference on smooth pairs (levels = 2, 3 trials) and the trials each accepted over both levels"""
    rref = R.build_ref(tmp_path_factory.mktemp("photo_robust_ref_for_keyframe_recover"))
    out = []
    for seed, px in ((1, 2.0), (2, 3.0)):
        s1, s2, _ = U.smooth_pair(seed, px)
        rec, lv = R.ref_run(rref, s1, s2, np.zeros(8, np.float32), 2, max_iterations=3)
        acc = int(lv[0]["px"]["accepted"].sum())
        assert acc > 0 and not rec[0]["px"]["flags"] & (U.SINGULAR | U.DEGENERATE | U.FEW_PIXELS)
        out.append((rec[0].copy(), acc))
    return out


def _zero_reloc():
    z = np.zeros(1, O.ORELOC)
    z["target"] = -2
    return z[0]


def _reloc(flags, rec=None):
    r = np.zeros(1, O.ORELOC)
    r["rv"]["flags"] = flags
    if rec is not None:
        r["rv"]["rec"] = rec
        r["rv"]["key_px"] = rec["px"]["offsets_px"]
    return r[0]


def test_layout():
    """offsets and sizes of hnet_keyframe_measure_recover as _capi lays it out (the reference's static_asserts pin them against include/hnet.h) and the
    new flags: bits of their own, REATTACHED inside the wider mask only"""
    d = _capi.KEYFRAME_MEASURE_RECOVER_DTYPE
    assert d.itemsize == 4488 and d.fields["m"][1] == 0 and d.fields["reloc"][1] == 2448
    assert d.fields["m"][0] == _capi.KEYFRAME_MEASURE_DTYPE and d.fields["reloc"][0] == _capi.KEYFRAME_RELOC_ORIENTED_DTYPE and d.fields["reloc"][0].itemsize == 2040
    assert (_capi.KFM_FROM_RELOC, _capi.KFM_REATTACHED) == (65536, 131072) == (FR.FROM_RELOC, FR.REATTACHED)
    assert _capi.KFMR_UNUSABLE == _capi.KFM_UNUSABLE | 131072 == FR.UNUSABLE and not _capi.KFM_UNUSABLE & (65536 | 131072)
    assert not (65536 | 131072) & (_capi.KFM_NOT_SELECTED | 15)


def test_usable_recover_every_reason_and_pair(lib):
    """every reason on an input of its own; every pair of reasons: the first in the header's order wins - FIRST, TRACK_LOST (LOST and not RECOVERED),
    REATTACHED (RECOVERED and RL_ATTACHED), TRACK_GAP, PREV_NOT_MEASURED; a RETRACKED record carries no reason of its own; without RECOVERED the function
    is hnet_kfm::usable on every input"""
    u = lib.filters_keyframe_recover_ref_usable
    lost, rec = _capi.KF_MSE_ABOVE_MAX | _capi.KF_BRIDGED, _capi.KF_RECOVERED
    base = dict(had_key=1, track=0, reloc=0, prev_ok=1)
    defects = [("first", FK.FIRST, dict(had_key=0)), ("lost", FK.TRACK_LOST, dict(track=lost, reloc=_capi.RL_NO_CANDIDATE)),
               ("reattached", FR.REATTACHED, dict(track=lost | rec, reloc=_capi.RL_ATTACHED)), ("gap", FK.TRACK_GAP, dict(gap=1)),
               ("prev", FK.PREV_NOT_MEASURED, dict(prev_ok=0))]

    def run(kw):
        a = dict(base)
        gap = kw.get("gap", 0)
        a.update({k: v for k, v in kw.items() if k != "gap"})
        return u(a["had_key"], a["track"] | (_capi.KF_GAP if gap else 0), a["reloc"], a["prev_ok"])

    assert run({}) == 0
    for name, bit, kw in defects:
        assert run(kw) == bit, name
    for j, (name, bit, kw) in enumerate(defects):
        for name2, bit2, kw2 in defects[j + 1:]:
            if set(kw) & set(kw2):
                continue
            both = dict(kw)
            both.update(kw2)
            assert run(both) == bit, (name, name2)
    # lost + reattached share their arguments: the two are exclusive by RECOVERED, whatever the relocalise's flags say
    assert u(1, lost, _capi.RL_ATTACHED, 1) == FK.TRACK_LOST and u(1, lost | rec, _capi.RL_RETRACKED, 1) == 0
    assert u(1, lost | rec | _capi.KF_GAP, _capi.RL_RETRACKED, 1) == FK.TRACK_GAP and u(1, lost | rec, _capi.RL_RETRACKED, 0) == FK.PREV_NOT_MEASURED
    for had in (0, 1):
        for tf in (0, _capi.KF_GAP, _capi.KF_STOPPED, _capi.KF_GAP | _capi.KF_NON_FINITE, _capi.KF_REKEYED | _capi.KF_LOW_OVERLAP):
            for rf in (0, _capi.RL_ATTACHED, _capi.RL_RETRACKED, _capi.RL_NO_CANDIDATE):
                for po in (0, 1):
                    assert u(had, tf, rf, po) == lib.filters_keyframe_recover_ref_plain_usable(had, tf, po)


def test_next_prev_ok_recover(lib):
    """for every LOST reason x {not recovered, RETRACKED, ATTACHED}: 0 only for LOST without RECOVERED; a record that is not lost gives 1; without
    RECOVERED it is hnet_kfm::next_prev_ok"""
    nx = lib.filters_keyframe_recover_ref_next_prev_ok
    for bit in LOST_BITS:
        for extra in (0, _capi.KF_BRIDGED, _capi.KF_BRIDGED | _capi.KF_REKEYED, _capi.KF_GAP):
            assert nx(bit | extra) == 0 == lib.filters_keyframe_recover_ref_plain_next_prev_ok(bit | extra)
            assert nx(bit | extra | _capi.KF_RECOVERED) == 1              # RETRACKED and ATTACHED alike: the record does not tell them apart, nor need it
    for tf in (0, _capi.KF_FIRST | _capi.KF_REKEYED, _capi.KF_GAP, _capi.KF_REKEYED | _capi.KF_MAX_AGE):
        assert nx(tf) == 1 == lib.filters_keyframe_recover_ref_plain_next_prev_ok(tf)


def test_measure_recover_off_is_measure(lib, good):
    """recovery off (no RECOVERED in the record, whatever the relocalise record holds): every output of measure_recover equals hnet_kfm::measure's bit for
    bit, on 7v's 40 random key pairs and on each unusable input"""
    (rec, acc), (rec2, acc2) = good
    o = FK.mopts()
    for seed in range(40):
        kp = synth.true_offsets(seed, 30.0).astype(np.float32)
        r = rec.copy()
        r["px"]["offsets_px"] = synth.true_offsets(seed + 100, 30.0).astype(np.float32)
        for rl in (_zero_reloc(), _reloc(_capi.RL_RETRACKED, rec2), _reloc(_capi.RL_ATTACHED, rec2)):
            a = FR.ref_measure(lib, 1, kp, 1, tk._track(r), acc, rl, acc2, o)
            b = FR.plain_measure(lib, 1, kp, 1, tk._track(r), acc, o)
            assert a[0] == b[0] == 1 and a[4] == b[4] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:4], b[1:4])), seed
    kp = synth.true_offsets(3, 4.0).astype(np.float32)
    line = np.array([0, 0, 10, 5, 20, 10, 30, 15], np.float32) - KU.P4.astype(np.float32)
    for had, key, po, tf, ac in ((0, kp, 1, 0, acc), (1, kp, 1, _capi.KF_STOPPED, acc), (1, kp, 1, _capi.KF_GAP, acc), (1, kp, 0, 0, acc), (1, line, 1, 0, acc), (1, kp, 1, 0, 0)):
        a = FR.ref_measure(lib, had, key, po, tk._track(rec, tf), ac, _reloc(_capi.RL_RETRACKED, rec2), acc2, o)
        b = FR.plain_measure(lib, had, key, po, tk._track(rec, tf), ac, o)
        assert a[0] == b[0] == 0 and a[4] == b[4] != 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:4], b[1:4]))


def test_measure_recover_retracked(lib, good):
    """RECOVERED with RL_RETRACKED: z_px = relative_z(key_px before, the relocalise record's offsets), R_px and the packed record are refine_measurement's
    on THAT record with ITS accepted count (the track's own record, lost, plays no part), and FROM_RELOC is set; an ATTACHED record is REATTACHED and
    writes nothing; the relocalise record's own defects are refine_measurement's reasons without FROM_RELOC"""
    (rec, acc), (rec2, acc2) = good
    o = FK.mopts(cov_scale=2.0)
    kp = synth.true_offsets(3, 4.0).astype(np.float32)
    lost = rec.copy()
    lost["px"]["flags"] |= U.DEGENERATE
    lost["px"]["mse"] = 900.0
    tr = tk._track(lost, _capi.KF_STOPPED | _capi.KF_BRIDGED | _capi.KF_RECOVERED, key_px=kp)
    ok, z, r_px, m72, fl = FR.ref_measure(lib, 1, kp, 1, tr, 0, _reloc(_capi.RL_RETRACKED, rec2), acc2, o)
    assert ok == 1 and fl == FR.FROM_RELOC
    assert z.tobytes() == FR.ref_relative_z(lib, kp, rec2["px"]["offsets_px"]).tobytes() and m72[:8].tobytes() == z.tobytes()
    # refine_measurement on the relocalise's record: hnet_kfm::measure on a plain track record that carries it gives the same R_px
    okp, zp, r_pxp, m72p, flp = FR.plain_measure(lib, 1, kp, 1, tk._track(rec2), acc2, o)
    assert okp == 1 and r_px.tobytes() == r_pxp.tobytes() and m72.tobytes() == m72p.tobytes() and z.tobytes() == zp.tobytes()
    assert FR.ref_measure(lib, 1, np.zeros(8), 1, tr, 0, _reloc(_capi.RL_RETRACKED, rec2), acc2, o)[1].tobytes() == rec2["px"]["offsets_px"].tobytes()
    ok, z, r_px, m72, fl = FR.ref_measure(lib, 1, kp, 1, tr, acc, _reloc(_capi.RL_ATTACHED, rec2), acc2, o)
    assert ok == 0 and fl == FR.REATTACHED and (z == 7.0).all() and (r_px == 7.0).all() and (m72 == 7.0).all()
    ok, _, _, _, fl = FR.ref_measure(lib, 1, kp, 1, tr, acc, _reloc(_capi.RL_RETRACKED, rec2), 0, o)
    assert ok == 0 and fl == FK.NO_STEP                                            # the SECOND alignment's count is the one that is read
    ok, _, _, _, fl = FR.ref_measure(lib, 1, kp, 1, tr, acc, _reloc(_capi.RL_RETRACKED, rec2), acc2, FK.mopts(max_mse=float(rec2["px"]["mse"]) * 0.999))
    assert ok == 0 and fl == FK.MSE_ABOVE_MAX


def _fs(lib, ses):
    """a RefFilterSession around the keyframe state and prev_ok of a test_filters_keyframe_cpu session (no map; the stub aligner needs no images)"""
    fs = FR.RefFilterSession(lib, 0)
    fs.ses.state[0], fs.prev_ok = ses["key"][0], int(ses["prev_ok"][0])
    return fs


@pytest.mark.parametrize("iters", [1, 3])
def test_null_recover_is_iterated_update_keyframe_measured(lib, good, iters):
    """a null recover option on every path of tests/test_filters_keyframe_cpu.py: the feature off, FIRST, LOST, GAP, no measured previous key_px, IF_NONE,
    a closed reference gate, a NIS gate that refuses everything, a singular S of the network's own, and the applied paths under both `when`: state,
    return value, innovation and photometric records, the measure record and the session equal iterated_update_keyframe_measured's byte for byte; the
    relocalise record is zero_reloc (zeros with the feature off) and the relocaliser is never called"""
    p, st, net, ses, rec, acc = tk._setup(good[0], 20 + iters, iters)
    sc = tg._script([0.5] * iters)
    o = FK.mopts()
    lost = rec.copy()
    lost["px"]["flags"] |= U.DEGENERATE
    nokey, notprev = FK.new_session(), ses.copy()
    notprev["prev_ok"] = 0
    zs = st.copy()
    zs["cov"] = 0.0
    znet = net.copy()
    znet[:, 8:] = 0.0
    cases = [("off", ses, rec, False, None, 0.0, 1, st, net), ("first", nokey, rec, False, o, 0.0, 1, st, net), ("lost", ses, lost, False, o, 0.0, 1, st, net),
             ("gap", ses, rec, True, o, 0.0, 1, st, net), ("prev", notprev, rec, False, o, 0.0, 1, st, net),
             ("if-none", ses, rec, False, FK.mopts(when=FK.IF_NONE), 0.0, 1, st, net), ("closed-unusable", nokey, rec, False, o, 0.0, 0, st, net),
             ("nis", ses, rec, False, o, 1e-30, 1, st, net), ("singular", ses, rec, False, o, 0.0, 1, zs, znet),
             ("applied", ses, rec, False, FK.mopts(cov_scale=3.0), 0.0, 1, st, net), ("applied-closed", ses, rec, False, FK.mopts(cov_scale=3.0), 0.0, 0, st, net),
             ("applied-if-none", ses, rec, False, FK.mopts(cov_scale=3.0, when=FK.IF_NONE), 0.0, 0, st, net)]
    frame = np.zeros((224, 320), np.uint8)
    applied = 0
    for name, s0, r0, gap, oo, max_nis, gate, st0, net0 in cases:
        a, b = _fs(lib, s0), _fs(lib, s0)
        ra = a.step(st0, p, net0, gate, max_nis, oo, None, None, frame, gap=gap, measured=False, align_rec=r0, accepted=acc, script=sc, max_ratio=2.0)
        rb = b.step(st0, p, net0, gate, max_nis, oo, None, None, frame, gap=gap, measured=True, align_rec=r0, accepted=acc, script=sc, max_ratio=2.0)
        assert ra["state"].tobytes() == rb["state"].tobytes() and ra["updates"] == rb["updates"], name
        assert ra["innov"].tobytes() == rb["innov"].tobytes() and ra["prec"].tobytes() == rb["prec"].tobytes(), name
        assert ra["rec"]["m"].tobytes() == rb["rec"]["m"].tobytes() and a.snapshot() == b.snapshot(), name
        assert list(ra["counts"]) == list(rb["counts"]) and ra["counts"][2] == 0, name
        want = np.zeros(1, O.ORELOC)[0] if oo is None else _zero_reloc()
        assert ra["rec"]["reloc"].tobytes() == want.tobytes(), name
        applied += int(bool(ra["rec"]["m"]["flags"] & FK.APPLIED))
    assert applied == 3


def _by_hand(before, frame, name, tab, step_px):
    """RefRecoverSession.track_recover on a clone of the session as it was, with the record's step_px"""
    h = before.ses.clone()
    o = KR.recover_opts(KR.track_opts(name), KR.reloc_opts(name))
    out, what = h.track_recover(frame, step_px, o, tab)
    return h, out, what


@pytest.mark.parametrize("name", KR.ROWS)
def test_rows(lib, tab, name):
    """7u's four rows over seeds 1, 2, 5, 11 through the host loop with the host reference alignment and the host relocalise, the rows' steps as the
    filter's offset states, a network that applies nothing, cov_scale = 1.  At every frame the loop equals RefRecoverSession.track_recover called by
    hand with the record's step_px on the bytes of track, reloc, keyframe state, map state, entries and images.  The rows' table: FIRST; on the
    kidnapped frame of the rows without a map LOST and RECOVERED, RETRACKED, FROM_RELOC and APPLIED without a NIS gate, NIS_REJECTED under max_nis =
    20 (the camera jumped), z_px = the relocalise's key_px within 7u's gate of the true pose; the next frame TRACKED and APPLIED.  With a map: the
    constant frame TRACK_LOST and prev_ok 0, the far frame REATTACHED with nothing applied and the filter state byte-equal to the run without a keyframe
    update, the frame after it APPLIED.  z_px of the frame after the recovery lies within twice the row's worst measured distance from the true relative
    pose (filters_keyframe_recover_util.NEXT_Z); today's code has no measurement on either frame: TRACK_LOST, then PREV_NOT_MEASURED."""
    for k, seed in enumerate(KR.SEEDS):
        r = KR.row(name, seed)

        def check(i, before, after, out, r=r):
            h, want, what = _by_hand(before, r["frames"][i], name, tab, out["rec"]["m"]["step_px"])
            assert out["rec"]["m"]["track"].tobytes() == want["track"].tobytes(), (seed, i)
            assert out["rec"]["reloc"].tobytes() == want["reloc"].tobytes(), (seed, i)
            assert after.ses.snapshot() == h.snapshot(), (seed, i)
            assert out["rec"]["m"]["step_px"].tobytes() == FR.row_step(r, i).astype(np.float32).tobytes()
            assert out["counts"][2] == (0 if what == KR.NOT_LOST else 1)

        outs = FR.run_row(lib, tab, name, seed, check=check)
        fl = [int(o["rec"]["m"]["flags"]) for o in outs]
        tf = [int(o["rec"]["m"]["track"]["flags"]) for o in outs]
        rf = [int(o["rec"]["reloc"]["rv"]["flags"]) for o in outs]
        lost, nxt, const = r["lost"], r["next"], r["constant"]
        assert fl[0] == FK.ASKED | FK.FIRST and outs[0]["updates"] == 0
        plain = FR.ref_row(lib, name, seed, recover=False)
        pfl = [int(o["rec"]["m"]["flags"]) for o in plain]
        assert pfl[lost] == FK.ASKED | FK.TRACK_LOST and pfl[nxt] == FK.ASKED | FK.PREV_NOT_MEASURED      # today: no measurement on two frames
        if const is None:
            assert fl[lost] == FK.ASKED | FK.APPLIED | FR.FROM_RELOC and tf[lost] & _capi.KF_LOST and tf[lost] & _capi.KF_RECOVERED and rf[lost] == _capi.RL_RETRACKED
            assert outs[lost]["updates"] == 1 and outs[lost]["rec"]["m"]["innov"]["nis"] > 20.0
            z = outs[lost]["rec"]["m"]["z_px"]
            assert z.tobytes() == outs[lost]["rec"]["reloc"]["rv"]["key_px"].tobytes()              # the previous key_px is zero
            assert S.worst_px(z, r["pose"]) <= KR.gate(name)
            gated = FR.ref_row(lib, name, seed, max_nis=20.0)
            g = gated[lost]["rec"]["m"]
            assert g["flags"] == FK.ASKED | FK.NIS_REJECTED | FR.FROM_RELOC and g["innov"]["flag"] == FK.INN_REJECTED and gated[lost]["updates"] == 0
            assert gated[nxt]["rec"]["m"]["flags"] == FK.ASKED | FK.APPLIED                      # prev_ok stayed 1
        else:
            assert fl[const] == FK.ASKED | FK.TRACK_LOST and not tf[const] & _capi.KF_RECOVERED and rf[const] & _capi.RL_NO_CANDIDATE
            assert fl[lost] == FK.ASKED | FR.REATTACHED and tf[lost] & _capi.KF_RECOVERED and rf[lost] == _capi.RL_ATTACHED and outs[lost]["updates"] == 0
            assert pfl[const] == FK.ASKED | FK.TRACK_LOST
            # REATTACHED rather than PREV_NOT_MEASURED: prev_ok was 0 on that frame
            off = FR.RefFilterSession(lib, KR.capacity(name)).step(FK.row_state(FR.row_step(r, lost), FR.row_time(lost)), FR.row_params(), FR.row_net(), 0, 0.0,
                                                                   None, None, None, r["frames"][lost])
            assert outs[lost]["state"].tobytes() == off["state"].tobytes()
            for i in range(1, const):
                assert fl[i] == FK.ASKED | FK.APPLIED, (seed, i)
        assert fl[nxt] == FK.ASKED | FK.APPLIED and not tf[nxt] & (_capi.KF_LOST | _capi.KF_RECOVERED) and outs[nxt]["updates"] == 1
        err = FR.next_z_error(name, seed, outs[nxt]["rec"]["m"]["z_px"])
        print(f"{name}, seed {seed}: flags {[hex(x) for x in fl]}; z_px of the frame after the recovery {err:.4f} px off the true relative pose "
              f"(gate {FR.next_z_gate(name):.4f}); today's code: {[hex(x) for x in pfl]}")
        assert err <= FR.next_z_gate(name) and abs(err - FR.NEXT_Z[name][k]) <= 1e-4


def test_filters_keyframe_recover_check_under_asan_ubsan(tmp_path):
    """the rule on heap records of exact size and one recovered frame through the host loop under AddressSanitizer + UBSan: a stand-alone program;
    nothing loaded into python is sanitized"""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    exe = str(tmp_path / "filters_keyframe_recover_check_san.bin")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *U.HOST_FLAGS, *san, os.path.join(ROOT, "tests", "cpp", "filters_keyframe_recover_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "filters keyframe recover check: ok" in r.stdout, r.stdout
