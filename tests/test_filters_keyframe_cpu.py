"""CPU: the keyframe track as an in-step filter measurement on the host (include/hnet_keyframe_measure.h; include/hnet.h
hnet_filters_set_keyframe_measure) through tests/cpp/filters_keyframe_ref.cpp: the layouts and defaults, z against a numpy float64
restatement, every UNUSABLE reason on an input of its own and in the order the header tests them, hnet_ekf::iterated_update_keyframe_measured with a stub
aligner on each of its paths - byte for byte against iterated_update_photo_gated where no keyframe measurement is applied, against update and
reset_4pt_offset called by hand where one is - the telescoping row on the out-and-back path, and the stand-alone program
tests/cpp/filters_keyframe_check.cpp under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filters_keyframe_util as FK
import keyframe_util as KU
import photo_align_util as U
import photo_robust_util as R
import test_filters_innov_cpu as ti
import test_filters_photo_gate_cpu as tg
from cuahn_vio_amd import _capi, synth

ROOT = U.ROOT
# measured worst over the 40 pairs of test_z_matches_numpy, max |z - numpy| / max |numpy|: 5.0e-08 (z is rounded to fp32).  Gate: 10 x
MEASURED_Z = 5.0e-08


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return FK.build_ref(tmp_path_factory.mktemp("filters_keyframe_ref"))


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    """a level-0 record of the host robust reference on a smooth pair (levels = 2, 3 trials) and the trials accepted over both levels"""
    rref = R.build_ref(tmp_path_factory.mktemp("photo_robust_ref_for_keyframe_measure"))
    s1, s2, _ = U.smooth_pair(1, 2.0)
    rec, lv = R.ref_run(rref, s1, s2, np.zeros(8, np.float32), 2, max_iterations=3)
    acc = int(lv[0]["px"]["accepted"].sum())
    assert acc > 0 and not rec[0]["px"]["flags"] & (U.SINGULAR | U.DEGENERATE | U.FEW_PIXELS)
    return rec[0].copy(), acc


def test_layouts_and_defaults(lib):
    """hnet_keyframe_measure and hnet_keyframe_measure_opts as _capi lays them out (the reference's static_asserts pin them against include/hnet.h); the
    defaults leave cov_scale 0, which the validity test refuses: the caller must choose it"""
    m = _capi.KEYFRAME_MEASURE_DTYPE
    assert m.itemsize == 2448 and m.fields["step_px"][1] == 1720 and m.fields["z_px"][1] == 1752 and m.fields["r_px"][1] == 1784
    assert m.fields["innov"][1] == 1784 + 512 and m.fields["flags"][1] == 2440 and m.fields["pad"][1] == 2444
    assert C.sizeof(_capi.KeyframeMeasureOpts) == 120 and _capi.KeyframeMeasureOpts.cov_scale.offset == 88 and _capi.KeyframeMeasureOpts.when.offset == 112
    assert C.sizeof(_capi.KeyframeMeasureStats) == 48
    assert (_capi.KFM_ASKED, _capi.KFM_APPLIED, _capi.KFM_NIS_REJECTED, _capi.KFM_S_SINGULAR) == (1, 2, 4, 8)
    assert _capi.KFM_UNUSABLE == FK.UNUSABLE and not _capi.KFM_UNUSABLE & (_capi.KFM_NOT_SELECTED | 15)
    d = _capi.KeyframeMeasureOpts()
    lib.filters_keyframe_ref_default_opts(C.byref(d))
    assert bytes(d.track) == bytes(_default_track(lib)) and (d.cov_scale, d.sigma_floor_px, d.max_mse, d.when, d.pad) == (0.0, 0.05, 0.0, FK.ALWAYS, 0)
    assert not lib.filters_keyframe_ref_opts_valid(C.byref(d))
    ok = lambda **kw: lib.filters_keyframe_ref_opts_valid(C.byref(FK.mopts(**kw)))
    assert ok() and ok(when=FK.IF_NONE) and ok(sigma_floor_px=0.0) and ok(max_mse=3.0) and ok(levels=1) and ok(max_age=3)
    for kw in (dict(cov_scale=0.0), dict(cov_scale=-1.0), dict(cov_scale=float("nan")), dict(cov_scale=float("inf")), dict(sigma_floor_px=-0.1),
               dict(sigma_floor_px=float("nan")), dict(max_mse=-1.0), dict(max_mse=float("inf")), dict(when=2), dict(when=-1), dict(levels=0), dict(levels=5),
               dict(auto_rekey=2), dict(max_age=-1), dict(rekey_overlap=1.5), dict(huber_k=-1.0)):
        assert not ok(**kw), kw


def _default_track(lib):
    kref_opts = _capi.KeyframeOpts()
    kf = C.CDLL(lib._name)
    kf.keyframe_ref_default_opts(C.byref(kref_opts))
    return kref_opts


def test_z_matches_numpy(lib):
    """z = corners(H(key_px_curr) . H(key_px_prev)^-1) - p4 (fp32 out) against numpy float64 with the DLT solved by LAPACK, on 40 random pairs up to 30 px:
    within 10 x MEASURED_Z; equal keys give zeros, a zero previous key the current one; a previous key without a homography writes nothing"""
    worst = 0.0
    for seed in range(40):
        kp, kc = synth.true_offsets(seed, 30.0).astype(np.float32), synth.true_offsets(seed + 100, 30.0).astype(np.float32)
        got = FK.ref_relative_z(lib, kp, kc)
        want = FK.np_relative_z(kp, kc)
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
        assert np.abs(FK.ref_relative_z(lib, kp, kp)).max() <= 1e-5
        assert FK.ref_relative_z(lib, np.zeros(8), kc).tobytes() == kc.tobytes()
    print(f"z, header vs numpy float64, worst relative difference: {worst:.3e}")
    assert worst <= 10 * MEASURED_Z
    line = np.array([0, 0, 10, 5, 20, 10, 30, 15], np.float32) - KU.P4.astype(np.float32)    # all four corners on one line: no homography, no inverse
    assert FK.ref_relative_z(lib, line, np.zeros(8)) is None
    assert FK.ref_relative_z(lib, np.full(8, np.nan), np.zeros(8)) is None and FK.ref_relative_z(lib, np.zeros(8), np.full(8, np.inf)) is None


def _track(rec, flags=0, key_px=None):
    t = np.zeros(1, FK.TRACK)
    t["rec"] = rec
    t["flags"] = flags
    t["key_px"] = rec["px"]["offsets_px"] if key_px is None else key_px
    return t


def test_every_unusable_reason_in_order(lib, good):
    """one input per reason: exactly its bit and nothing written; then inputs with several defects: the first in the header's order wins - FIRST, TRACK_LOST,
    TRACK_GAP, PREV_NOT_MEASURED, NO_INVERSE, then 7o's BAD_K_NET_COV, STOPPED, NO_STEP, MSE_ABOVE_MAX, NO_FACTOR, NON_FINITE"""
    rec, acc = good
    key_prev = synth.true_offsets(3, 4.0).astype(np.float32)
    line = np.array([0, 0, 10, 5, 20, 10, 30, 15], np.float32) - KU.P4.astype(np.float32)
    o = FK.mopts()
    ok, z, r_px, out72, flags = FK.ref_measure(lib, 1, key_prev, 1, _track(rec), acc, o)
    assert ok == 1 and flags == 0 and z.tobytes() == FK.ref_relative_z(lib, key_prev, rec["px"]["offsets_px"]).tobytes()
    assert out72[:8].tobytes() == z.tobytes() and out72[8:].tobytes() == (r_px.reshape(64) / 10.0).astype(np.float32).tobytes()
    assert (r_px == r_px.T).all() and (np.diag(np.linalg.cholesky(r_px)) > 0).all()
    flagged = rec.copy()
    flagged["px"]["flags"] |= U.SINGULAR
    stripes = rec.copy()
    stripes["info10"][:] = 0.0
    stripes["px"]["info"][:] = 0.0                                               # the model off and a zero information matrix: no factor
    huge = rec.copy()
    huge["px"]["mse"] = 1e308
    # (had_key, key_prev, prev_ok, track, accepted, opts, k) in the order of the reasons; case j carries the defects of every case behind it as well
    defects = [
        ("first", FK.FIRST, dict(had_key=0)),
        ("lost", FK.TRACK_LOST, dict(tflags=_capi.KF_STOPPED | _capi.KF_REKEYED | _capi.KF_BRIDGED)),
        ("gap", FK.TRACK_GAP, dict(tflags=_capi.KF_GAP)),
        ("prev", FK.PREV_NOT_MEASURED, dict(prev_ok=0)),
        ("inverse", FK.NO_INVERSE, dict(key_prev=line)),
        ("k", FK.BAD_K, dict(k=float("nan"))),
        ("stopped", FK.STOPPED, dict(rec=flagged)),
        ("no-step", FK.NO_STEP, dict(accepted=0)),
        ("mse", FK.MSE_ABOVE_MAX, dict(o=FK.mopts(max_mse=float(rec["px"]["mse"]) * 0.999))),
        ("factor", FK.NO_FACTOR, dict(rec=stripes)),
        ("non-finite", FK.NON_FINITE, dict(rec=huge, o=FK.mopts(cov_scale=1e10))),
    ]

    def run(kw):
        a = dict(had_key=1, key_prev=key_prev, prev_ok=1, tflags=0, rec=rec, accepted=acc, o=o, k=10.0)
        a.update(kw)
        return FK.ref_measure(lib, a["had_key"], a["key_prev"], a["prev_ok"], _track(a["rec"], a["tflags"]), a["accepted"], a["o"], a["k"])

    for name, bit, kw in defects:
        ok, z, r_px, out72, flags = run(kw)
        assert ok == 0 and flags == bit, (name, flags)
        assert (z == 7.0).all() and (r_px == 7.0).all() and (out72 == 7.0).all(), name
    # the order: a defect together with every defect tested before it that does not share its argument
    for j, (name, bit, kw) in enumerate(defects):
        for name2, bit2, kw2 in defects[j + 1:]:
            if set(kw) & set(kw2):
                continue
            both = dict(kw)
            both.update(kw2)
            ok, _, _, _, flags = run(both)
            assert ok == 0 and flags == bit, (name, name2, flags)
    # a LOST bit wins over GAP in one record
    ok, _, _, _, flags = run(dict(tflags=_capi.KF_GAP | _capi.KF_NON_FINITE))
    assert flags == FK.TRACK_LOST
    assert [lib.filters_keyframe_ref_selected(w, u) for w, u in ((0, 0), (0, 3), (0, -1), (1, 0), (1, 1), (1, -2))] == [1, 1, 0, 1, 0, 0]


def _setup(good, seed, iters=3, key_spread=4.0):
    """a state, a network script around its prior, a session that holds a keyframe with a measured key_px, and a stub record whose offsets lie near
    compose(step of the posterior-ish state, key_px): an alignment that ended near what the filter predicts"""
    rng = np.random.default_rng(seed)
    p = ti._params()
    st = ti._state(rng)
    net = np.stack([ti._net(rng, st, 0.5) for _ in range(iters)])
    ses = FK.new_session()
    ses["key"]["has_key"], ses["key"]["age"], ses["key"]["keyframes"] = 1, 2, 1
    ses["key"]["key_px"] = synth.true_offsets(seed, key_spread).astype(np.float32)
    ses["key"]["h_origin_key"] = np.eye(3)
    ses["prev_ok"] = 1
    rec, acc = good
    rec = rec.copy()
    prior = (st["offset"][0][:, :2].reshape(8) * FK.F).astype(np.float32)
    rec["px"]["offsets_px"] = (KU.np_compose(prior, ses["key"]["key_px"][0]) + 0.2 * rng.standard_normal(8)).astype(np.float32)
    return p, st, net, ses, rec, acc


def _same(a, g):
    return a["state"].tobytes() == g[0].tobytes() and a["updates"] == g[1] and a["innov"].tobytes() == g[2].tobytes() and a["prec"].tobytes() == g[3].tobytes()


@pytest.mark.parametrize("iters", [1, 3])
def test_no_measurement_is_iterated_update_photo_gated(lib, good, iters):
    """every path that applies no keyframe measurement leaves, byte for byte, the state, the return value and the innovation and photometric records of
    iterated_update_photo_gated (update_offset = 1 on the last iteration is invisible behind the reset): the feature off (the aligner is never called, the
    record zero); on with a session without a keyframe (FIRST), a LOST record, GAP, no measured previous key_px, a refused NIS, IF_NONE after applied
    updates, and a singular S of the network's own.  The keyframe session still advances as the track advances it."""
    p, st, net, ses, rec, acc = _setup(good, 20 + iters, iters)
    sc = tg._script([0.5] * iters)
    o = FK.mopts()
    want = FK.ref_gated(lib, st, p, net, 1, 0.0, sc, 2.0)
    off = FK.ref_iterated(lib, st, p, net, 1, 0.0, sc, 2.0, None, False, ses, align_rec=rec, accepted=acc)
    assert _same(off, want) and off["calls"] == want[4] == iters and off["align_calls"] == 0
    assert off["rec"].tobytes() == np.zeros(1, FK.MEASURE).tobytes() and off["session"].tobytes() == ses.tobytes()
    lost = rec.copy()
    lost["px"]["flags"] |= U.DEGENERATE
    nokey, notprev = FK.new_session(), ses.copy()
    notprev["prev_ok"] = 0
    cases = [("first", nokey, rec, False, o, 0.0, 1, FK.FIRST), ("lost", ses, lost, False, o, 0.0, 1, FK.TRACK_LOST), ("gap", ses, rec, True, o, 0.0, 1, FK.TRACK_GAP),
             ("prev", notprev, rec, False, o, 0.0, 1, FK.PREV_NOT_MEASURED), ("if-none", ses, rec, False, FK.mopts(when=FK.IF_NONE), 0.0, 1, FK.NOT_SELECTED),
             ("closed-unusable", nokey, rec, False, o, 0.0, 0, FK.FIRST)]
    for name, s0, r0, gap, oo, max_nis, gate, bit in cases:
        want = FK.ref_gated(lib, st, p, net, gate, max_nis, sc, 2.0)
        got = FK.ref_iterated(lib, st, p, net, gate, max_nis, sc, 2.0, oo, gap, s0, align_rec=r0, accepted=acc)
        assert _same(got, want), name
        assert got["rec"]["flags"] == FK.ASKED | bit and got["rec"]["pad"] == 0 and got["calls"] == iters, (name, int(got["rec"]["flags"]))
        assert got["align_calls"] == (0 if name in ("first", "closed-unusable") else 1)
        assert got["rec"]["innov"]["flag"] == FK.INN_NONE and got["rec"]["innov"]["iteration"] == iters and not got["rec"]["innov"]["r"].any()
        assert got["rec"]["step_px"].tobytes() == _posterior_step(lib, st, p, net, gate).tobytes(), name
        if bit != FK.NOT_SELECTED:
            assert not got["rec"]["z_px"].any() and not got["rec"]["r_px"].any()
        else:
            assert got["rec"]["z_px"].any() and got["rec"]["r_px"].any()            # usable, and kept out
        assert got["session"]["key"]["has_key"][0] == 1
        assert got["session"]["prev_ok"][0] == (0 if name == "lost" else 1), name
    # a NIS gate that refuses everything: the network's updates and the keyframe measurement alike
    want = FK.ref_gated(lib, st, p, net, 1, 1e-30, sc, 2.0)
    got = FK.ref_iterated(lib, st, p, net, 1, 1e-30, sc, 2.0, o, False, ses, align_rec=rec, accepted=acc)
    assert _same(got, want) and got["rec"]["flags"] == FK.ASKED | FK.NIS_REJECTED and got["rec"]["innov"]["flag"] == FK.INN_REJECTED and got["updates"] == 0
    # a singular S of the network's own (zero covariances on both sides): neither `when` applies
    zs = st.copy()
    zs["cov"] = 0.0
    znet = net.copy()
    znet[:, 8:] = 0.0
    want = FK.ref_gated(lib, zs, p, znet, 1, 0.0, sc, 2.0)
    for w in (FK.ALWAYS, FK.IF_NONE):
        got = FK.ref_iterated(lib, zs, p, znet, 1, 0.0, sc, 2.0, FK.mopts(when=w), False, ses, align_rec=rec, accepted=acc)
        assert want[1] == -1 and _same(got, want) and got["rec"]["flags"] == FK.ASKED | FK.NOT_SELECTED


def _posterior_step(lib, st, p, net, gate):
    """step_px of the state after the network's iterations, every update with update_offset = 1, by hand"""
    s = st.copy()
    if gate:
        for it in range(len(net)):
            ok, s = FK.ref_update(lib, s, p, net[it], 1, 0)
            assert ok == 1
    return FK.ref_step(lib, s)


@pytest.mark.parametrize("when,gate", [(FK.ALWAYS, 1), (FK.ALWAYS, 0), (FK.IF_NONE, 0)])
@pytest.mark.parametrize("iters", [1, 3])
def test_measurement_is_update_by_hand(lib, good, iters, when, gate):
    """the paths that apply one: the state equals, byte for byte, the network's updates called by hand with update_offset = 1 (when its reference gate is
    open), then update with measure's packed record against the state's own prior and update_offset = 0, then reset_4pt_offset; the aligner is called once
    with compose(step_px, key_px); the record holds the track's, z_px, R_px and hnet_ekf::innovation of the measurement on the posterior; the return value
    counts the update; the session's key_px is the record's offsets and prev_ok 1"""
    p, st, net, ses, rec, acc = _setup(good, 30 + iters, iters)
    o = FK.mopts(cov_scale=3.0, when=when)
    sc = tg._script([0.5] * iters)
    got = FK.ref_iterated(lib, st, p, net, gate, 0.0, sc, 2.0, o, False, ses, align_rec=rec, accepted=acc)
    post = st.copy()
    if gate:
        for it in range(iters):
            ok, post = FK.ref_update(lib, post, p, net[it], 1, 0)
            assert ok == 1
    step = FK.ref_step(lib, post)
    key_prev = ses["key"]["key_px"][0]
    assert got["align_calls"] == 1 and got["calls"] == iters and got["x0"].tobytes() == KU.ref_compose(C.CDLL(lib._name), step, key_prev).tobytes()
    r = got["rec"]
    assert r["step_px"].tobytes() == step.tobytes() and r["track"]["rec"].tobytes() == rec.tobytes() and r["track"]["start_px"].tobytes() == got["x0"].tobytes()
    assert r["track"]["flags"] == 0 and r["track"]["key_px"].tobytes() == rec["px"]["offsets_px"].tobytes() and r["track"]["age"] == 3
    ok, z, r_px, m72, fl = FK.ref_measure(lib, 1, key_prev, 1, r["track"], acc, o, p.k_net_cov)
    assert ok == 1 and fl == 0 and r["z_px"].tobytes() == z.tobytes() and r["r_px"].tobytes() == r_px.tobytes()
    ok, inn = FK.ref_innovation(lib, post, p, m72)
    inn["iteration"] = iters
    assert ok == 1 and r["innov"].tobytes() == inn.tobytes() and r["innov"]["flag"] == FK.INN_USED and np.isfinite(r["innov"]["nis"])
    ok, hand = FK.ref_update(lib, post, p, m72, 0, 1)
    assert ok == 1 and got["state"].tobytes() == hand.tobytes()
    assert got["state"].tobytes() != FK.ref_reset(lib, post).tobytes()              # the measurement moved the IMU block
    assert r["flags"] == FK.ASKED | FK.APPLIED and r["pad"] == 0 and got["updates"] == (iters if gate else 0) + 1
    assert np.all(got["state"]["offset"] == 0) and np.all(got["state"]["cov"][0][15:, :] == 0)
    assert got["session"]["key"]["key_px"][0].tobytes() == rec["px"]["offsets_px"].tobytes() and got["session"]["prev_ok"][0] == 1 and got["session"]["key"]["age"][0] == 3
    assert got["copy"] == 0
    # z is the consecutive-frame measurement: near the step the filter predicted (the stub record lies 0.2 px around the composed prior)
    assert np.abs(z - (st["offset"][0][:, :2].reshape(8) * FK.F)).max() < 3.0


def test_singular_keyframe_update(lib, good):
    """a zero state covariance, a closed reference gate and a zero R_px (mse = 0, no floor): S is singular, the state is the reset's alone, -1 - applied"""
    p, st, net, ses, rec, acc = _setup(good, 44, 2)
    zs = st.copy()
    zs["cov"] = 0.0
    zrec = rec.copy()
    zrec["px"]["mse"] = 0.0
    sc = tg._script([0.5, 0.5])
    got = FK.ref_iterated(lib, zs, p, net, 0, 0.0, sc, 2.0, FK.mopts(sigma_floor_px=0.0), False, ses, align_rec=zrec, accepted=acc)
    assert got["updates"] == -1 and got["rec"]["flags"] == FK.ASKED | FK.S_SINGULAR and got["rec"]["innov"]["flag"] == FK.INN_SINGULAR and np.isnan(got["rec"]["innov"]["nis"])
    assert got["state"].tobytes() == FK.ref_reset(lib, zs).tobytes()


@pytest.mark.parametrize("seed", FK.ROW_SEEDS)
def test_telescoping_row(lib, seed):
    """7p's out-and-back path, steps = truth + 0.3 px pseudo-noise as the filter's offsets, a network that applies nothing: the running composition of
    H(z_px) stays within 7p's gate (twice 0.0815 px) of the truth at EVERY frame - the errors telescope - while the plain composition of the noisy steps
    ends at least 3 gates off at frame 8.  Every measurement from frame 1 on is applied.  (DESIGN 7v holds the figures printed here)"""
    recs = FK.ref_row(lib, seed)
    worst, drift, per = FK.row_figures(recs, seed)
    print(f"seed {seed}: composition of H(z_px) worst {worst:.4f} px off (per frame {np.round(per, 4).tolist()}); composition of the noisy steps at frame 8: "
          f"{drift:.4f} px off = {drift / FK.ROW_GATE:.2f} gates; NIS {np.round(recs['innov']['nis'][1:], 3).tolist()}")
    assert recs["flags"][0] == FK.ASKED | FK.FIRST and all(int(f) == FK.ASKED | FK.APPLIED for f in recs["flags"][1:])
    assert worst <= FK.ROW_GATE
    assert drift >= KU.DRIFT_RATIO * FK.ROW_GATE
    # the telescope itself: the composition ends where the last key_px lies (no re-key on this path), to fp32 rounding of the z
    h = np.eye(3)
    for i in range(1, 9):
        h = FK.compose_running(h, recs[i]["z_px"])
        assert np.abs(KU.corners(h) - recs[i]["track"]["key_px"].astype(np.float64)).max() < 2e-5 * i, i


def test_keyframe_measure_header_under_asan_ubsan(tmp_path):
    """the header on synthetic records and scripted loops under AddressSanitizer + UBSan: a stand-alone program; nothing loaded into python is sanitized"""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    exe = str(tmp_path / "filters_keyframe_check_san.bin")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *U.HOST_FLAGS, *san, os.path.join(ROOT, "tests", "cpp", "filters_keyframe_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "filters keyframe check: z, 11 unusable cases, 6 loop paths (2 applied) ok" in r.stdout, r.stdout
