"""Tracking against a held keyframe on the host (include/hnet_keyframe.h, tests/cpp/keyframe_ref.cpp), no GPU: compose and decide against a
numpy float64 restatement, every LOST reason, every re-key reason and ORIGIN_RESTARTED each on an input of its own, the accuracy rows of the host
reference whose gates the GPU tests use, and the condition on the drift test's input."""
import numpy as np
import pytest

import keyframe_util as K
import photo_align_util as U
from cuahn_vio_amd import _capi, synth

# Measured (printed by test_compose_matches_numpy / test_decide_matches_numpy), each gated at 10 x the measurement: the header against the numpy float64
# restatement, worst difference relative to the largest entry.  compose ends in a rounding to fp32 (2^-24 = 6e-8 of the value at the most); the
# homographies of decide stay in double, and the restatement solves the 8 x 8 DLT system where the header evaluates its closed form.
MEASURED = {"compose": 4.9e-08, "h_origin": 2.9e-16}


@pytest.fixture(scope="module")
def kref(tmp_path_factory):
    return K.build_ref(tmp_path_factory.mktemp("keyframe_ref"))


def _rec(offsets=None, flags=0, mse=4.0, n_valid=70000, accepted=3):
    r = np.zeros(1, K.REC)
    r["px"]["offsets_px"] = np.zeros(8, np.float32) if offsets is None else offsets
    r["px"]["flags"], r["px"]["mse"], r["px"]["mse0"], r["px"]["n_valid"], r["px"]["n_valid0"] = flags, mse, 2 * mse, n_valid, n_valid
    r["px"]["trials"], r["px"]["accepted"], r["gain"] = 6, accepted, 1.0
    return r


def _state(key_px=None, h=None, age=2, keyframes=1):
    s = K.new_state()
    s["has_key"], s["age"], s["keyframes"] = 1, age, keyframes
    s["key_px"] = np.zeros(8, np.float32) if key_px is None else key_px
    s["h_origin_key"] = np.eye(3) if h is None else h
    return s


def _as_dict(s):
    return dict(has_key=int(s["has_key"][0]), age=int(s["age"][0]), keyframes=int(s["keyframes"][0]), key_px=s["key_px"][0].copy(), h_origin_key=s["h_origin_key"][0].copy())


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_layouts_and_default_opts(kref):
    import ctypes as C
    o = _capi.KeyframeOpts()
    kref.keyframe_ref_default_opts(C.byref(o))
    d = K.opts(max_iterations=6)
    assert bytes(o) == bytes(d) and (o.levels, o.auto_rekey, o.max_age, o.rekey_overlap, o.max_mse) == (3, 1, 0, 0.6, 0.0)
    assert kref.keyframe_ref_opts_valid(C.byref(o)) == 1
    for bad in (dict(levels=0), dict(levels=5), dict(rekey_overlap=1.5), dict(rekey_overlap=-0.1), dict(max_mse=-1.0), dict(max_mse=float("inf")), dict(auto_rekey=2),
                dict(max_age=-1), dict(huber_k=-1.0)):
        b = K.opts(**bad)
        assert kref.keyframe_ref_opts_valid(C.byref(b)) == 0, bad
    header = open(K.ROOT + "/include/hnet.h").read()
    for name in _capi.SYMBOLS[-6:]:
        assert "keyframe" in name and name in header


def test_compose_matches_numpy(kref):
    """the header's compose (fp32 out) against H(step) . H(key) by numpy in float64, over random offsets up to 30 px: within 10 x MEASURED; a zero step
    gives key_px back exactly, a zero key the step; failures write nothing"""
    worst = 0.0
    for seed in range(40):
        step, key = synth.true_offsets(seed, 6.0).astype(np.float32), synth.true_offsets(seed + 100, 30.0).astype(np.float32)
        got = K.ref_compose(kref, step, key)
        worst = max(worst, _rel(got, K.np_compose(step, key)))
        assert K.ref_compose(kref, np.zeros(8), key).tobytes() == key.tobytes()
        assert K.ref_compose(kref, step, np.zeros(8)).tobytes() == step.tobytes()
    print(f"compose, header vs numpy float64, worst relative difference: {worst:.3e}")
    assert worst <= 10 * MEASURED["compose"]
    p4 = K.P4.astype(np.float32)
    line = np.array([0, 0, 10, 5, 20, 10, 30, 15], np.float32) - p4                 # all four corners on one line: no homography
    nan = np.full(8, np.nan, np.float32)
    behind = np.array([0, 0, 0, 0, -700, -500, 0, 0], np.float32)                   # br pulled through the opposite corner: a corner's z turns negative
    zero = np.zeros(8, np.float32)
    for step, key in ((line, zero), (zero, line), (nan, zero), (zero, nan), (np.full(8, np.inf, np.float32), zero)):
        assert K.ref_compose(kref, step, key) is None
    fold = K.ref_compose(kref, behind, behind)
    assert fold is None or np.isfinite(fold).all()


CASES = {
    # name -> (state kwargs, start, record kwargs, opts kwargs, gap, flags expected)
    "tracked": (dict(), [1.0] * 8, dict(offsets=np.arange(8, dtype=np.float32) * 0.5), dict(), False, 0),
    "tracked-no-trial-accepted": (dict(), [0.0] * 8, dict(accepted=0, mse=0.0), dict(), False, 0),
    "gap": (dict(), [1.0] * 8, dict(), dict(), True, _capi.KF_GAP),
    "lost-no-start": (dict(key_px=np.full(8, 2.0, np.float32)), [np.nan] * 8, dict(flags=U.DEGENERATE, n_valid=0), dict(),
                      False, _capi.KF_NO_START | _capi.KF_REKEYED | _capi.KF_BRIDGED),
    "lost-stopped-singular": (dict(), [3.0] * 8, dict(flags=U.SINGULAR), dict(), False, _capi.KF_STOPPED | _capi.KF_REKEYED | _capi.KF_BRIDGED),
    "lost-stopped-few-pixels": (dict(), [3.0] * 8, dict(flags=U.FEW_PIXELS, n_valid=100), dict(), False, _capi.KF_STOPPED | _capi.KF_REKEYED | _capi.KF_BRIDGED),
    "lost-mse": (dict(), [3.0] * 8, dict(mse=50.0), dict(max_mse=40.0), False, _capi.KF_MSE_ABOVE_MAX | _capi.KF_REKEYED | _capi.KF_BRIDGED),
    "lost-mse-nan": (dict(), [3.0] * 8, dict(mse=float("nan")), dict(max_mse=40.0), False, _capi.KF_MSE_ABOVE_MAX | _capi.KF_REKEYED | _capi.KF_BRIDGED),
    "mse-not-judged-at-zero": (dict(), [3.0] * 8, dict(mse=1e9), dict(max_mse=0.0), False, 0),
    "lost-non-finite": (dict(), [3.0] * 8, dict(offsets=np.array([0, 0, np.inf, 0, 0, 0, 0, 0], np.float32)), dict(), False,
                        _capi.KF_NON_FINITE | _capi.KF_REKEYED | _capi.KF_BRIDGED),
    "lost-keeps-keyframe": (dict(key_px=np.full(8, 2.0, np.float32)), [3.0] * 8, dict(flags=U.SINGULAR), dict(auto_rekey=0), False, _capi.KF_STOPPED | _capi.KF_BRIDGED),
    "lost-no-start-keeps-keyframe": (dict(key_px=np.full(8, 2.0, np.float32)), [np.nan] * 8, dict(flags=U.DEGENERATE, n_valid=0), dict(auto_rekey=0), False,
                                     _capi.KF_NO_START),
    "rekey-low-overlap": (dict(), [1.0] * 8, dict(n_valid=40000), dict(), False, _capi.KF_LOW_OVERLAP | _capi.KF_REKEYED),
    "rekey-max-age": (dict(age=4), [1.0] * 8, dict(), dict(max_age=5), False, _capi.KF_MAX_AGE | _capi.KF_REKEYED),
    "max-age-not-yet": (dict(age=3), [1.0] * 8, dict(), dict(max_age=5), False, 0),
    "rekey-both": (dict(age=4), [1.0] * 8, dict(n_valid=40000), dict(max_age=5), False, _capi.KF_LOW_OVERLAP | _capi.KF_MAX_AGE | _capi.KF_REKEYED),
    "no-auto-rekey": (dict(age=9), [1.0] * 8, dict(n_valid=40000), dict(auto_rekey=0, max_age=5), False, 0),
    # origin -> keyframe sends the image to infinity along h[8]: H(key_px) . h_origin_key has h[8] = 0
    "origin-restarted": (dict(h=np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 0]])), [1.0] * 8, dict(), dict(), False, _capi.KF_ORIGIN_RESTARTED),
    "origin-restarted-non-finite": (dict(h=np.array([[1.0, 0, 0], [0, np.inf, 0], [0, 0, 1]])), [1.0] * 8, dict(), dict(), False, _capi.KF_ORIGIN_RESTARTED),
}


@pytest.mark.parametrize("name", list(CASES))
def test_decide_cases(kref, name):
    """every LOST reason, every re-key reason, GAP and ORIGIN_RESTARTED on an input of its own: the flags are the expected ones, and state, record and copy
    flag agree with the numpy restatement (integers and offsets exactly, the homographies within 10 x MEASURED)"""
    skw, start, rkw, okw, gap, want = CASES[name]
    s, r, o = _state(**skw), _rec(**rkw), K.opts(**okw)
    start = np.asarray(start, np.float32)
    ns, out, copy = K.ref_decide(kref, s, start, r, o, gap)
    ens, eout, ecopy = K.np_decide(_as_dict(s), start, r[0], o, gap)
    assert int(out["flags"][0]) == want == eout["flags"], (name, int(out["flags"][0]), want, eout["flags"])
    assert copy == ecopy == (1 if want & _capi.KF_REKEYED else 0)
    assert out["rec"].tobytes() == r.tobytes() and out["pad"][0] == 0 and ns["pad"][0] == 0
    assert (int(out["age"][0]), int(out["keyframes"][0]), float(out["overlap"][0])) == (eout["age"], eout["keyframes"], eout["overlap"])
    assert out["start_px"][0].tobytes() == start.tobytes() and out["key_px"][0].tobytes() == np.asarray(eout["key_px"], np.float32).tobytes()
    assert (int(ns["has_key"][0]), int(ns["age"][0]), int(ns["keyframes"][0])) == (1, ens["age"], ens["keyframes"])
    assert ns["key_px"][0].tobytes() == np.asarray(ens["key_px"], np.float32).tobytes()
    assert _rel(out["h_origin_curr"][0], eout["h_origin_curr"]) <= 10 * MEASURED["h_origin"] and out["h_origin_curr"][0][2, 2] == 1.0
    assert _rel(ns["h_origin_key"][0], ens["h_origin_key"]) <= 10 * MEASURED["h_origin"]
    if want & _capi.KF_REKEYED:
        assert not ns["key_px"][0].any() and ns["age"][0] == 0 and ns["keyframes"][0] == s["keyframes"][0] + 1
        assert ns["h_origin_key"][0].tobytes() == out["h_origin_curr"][0].tobytes()
    if name == "lost-no-start":                       # the bridge is the previous key_px
        assert out["key_px"][0].tobytes() == s["key_px"][0].tobytes()
    if name == "lost-keeps-keyframe":                 # the bridge is the start, and it becomes key_px
        assert ns["key_px"][0].tobytes() == start.tobytes() and ns["age"][0] == s["age"][0] + 1
    if name == "lost-no-start-keeps-keyframe":
        assert ns["key_px"][0].tobytes() == s["key_px"][0].tobytes()
    if want & _capi.KF_ORIGIN_RESTARTED:
        assert ns["h_origin_key"][0].tobytes() == np.eye(3).tobytes()


def test_decide_first(kref):
    """a session without a keyframe: FIRST | REKEYED, nothing of start or record is read, every byte of the output written"""
    s, r = K.new_state(), _rec(offsets=np.full(8, np.nan, np.float32), flags=U.SINGULAR)
    ns, out, copy = K.ref_decide(kref, s, np.full(8, np.nan, np.float32), r, K.opts(), True)
    want = np.zeros(1, K.TRACK)
    want["h_origin_curr"], want["keyframes"], want["flags"] = np.eye(3), 1, _capi.KF_FIRST | _capi.KF_REKEYED
    assert copy == 1 and out.tobytes() == want.tobytes()
    e = K.new_state()
    e["has_key"], e["keyframes"], e["h_origin_key"] = 1, 1, np.eye(3)
    assert ns.tobytes() == e.tobytes()


def test_decide_matches_numpy(kref):
    """decide on a chain of 30 random tracked frames with re-keys (max_age 4): the origin chain of the header against the numpy restatement, within 10 x
    MEASURED; the integers and offsets exactly"""
    o = K.opts(max_age=4)
    s = K.new_state()
    d = dict(has_key=0, age=0, keyframes=0, key_px=np.zeros(8, np.float32), h_origin_key=np.eye(3))
    worst = 0.0
    for i in range(30):
        x = synth.true_offsets(200 + i, 20.0).astype(np.float32)
        r = _rec(offsets=x, n_valid=60000 + i)
        s, out, copy = K.ref_decide(kref, s, x, r, o)
        d, eout, ecopy = K.np_decide(d, x, r[0], o, False)
        assert (copy, int(out["flags"][0]), int(out["age"][0]), int(out["keyframes"][0])) == (ecopy, eout["flags"], eout["age"], eout["keyframes"]), i
        worst = max(worst, _rel(out["h_origin_curr"][0], eout["h_origin_curr"]), _rel(s["h_origin_key"][0], d["h_origin_key"]))
    assert int(s["keyframes"][0]) == 8
    print(f"decide, header vs numpy float64, h_origin_curr / h_origin_key over 30 frames, worst relative difference: {worst:.3e}")
    assert worst <= 10 * MEASURED["h_origin"]


@pytest.mark.parametrize("name", list(K.ROWS))
def test_accuracy_rows(kref, name):
    """the host reference on the row's sequence over seeds 1, 2, 5, 11: worst distance of key_px from the true key -> curr offsets and of the corners of
    h_origin_curr from the true pose, over every frame.  The gates of keyframe_util.ROWS are twice these."""
    overlap, gate_key, gate_origin = K.ROWS[name]
    wk = wo = 0.0
    for seed in U.SEEDS:
        _, poses, _ = K.sequence(name, seed)
        recs = K.ref_row(kref, name, seed)
        rekeys = [i for i in range(1, len(recs)) if recs[i]["flags"] & _capi.KF_REKEYED]
        assert not (recs["flags"][1:] & (_capi.KF_LOST | _capi.KF_GAP | _capi.KF_ORIGIN_RESTARTED)).any(), (seed, recs["flags"])
        assert recs[0]["flags"] == _capi.KF_FIRST | _capi.KF_REKEYED
        if name == "translation-32":
            assert rekeys == [8] and recs[8]["flags"] == _capi.KF_REKEYED | _capi.KF_LOW_OVERLAP and recs[-1]["keyframes"] == 2 and recs[-1]["age"] == 2, (seed, rekeys)
        else:
            assert not rekeys and recs[-1]["age"] == 8 and recs[-1]["keyframes"] == 1, (seed, rekeys)
        a, b = K.worst_key_px(recs, poses), K.worst_origin_px(recs, poses)
        print(f"{name}, seed {seed}: key_px {a:.3e} px, corners of h_origin_curr {b:.3e} px off the truth at the worst frame")
        wk, wo = max(wk, a), max(wo, b)
    print(f"{name}: worst over the seeds: key_px {wk:.3e} px, h_origin_curr {wo:.3e} px; gates {gate_key:.3e}, {gate_origin:.3e}")
    assert wk <= gate_key and wo <= gate_origin


def test_drift_input_condition(kref):
    """out-and-back, frame 8 (the keyframe's pose): the host reference's key_px is within the gate of zero, and the plain chained sum of the same noisy
    steps is at least 3 gates off - otherwise the GPU drift test would show nothing"""
    gate = K.ROWS["out-and-back"][1]
    for seed in U.SEEDS:
        _, poses, steps = K.sequence("out-and-back", seed)
        assert not poses[8].any()
        recs = K.ref_row(kref, "out-and-back", seed)
        off, drift = float(np.abs(recs[8]["key_px"]).max()), float(np.abs(K.chained_sum(steps, 8)).max())
        print(f"seed {seed}: frame 8: key_px {off:.3e} px off zero, chained sum of the steps {drift:.4f} px off ({drift / gate:.1f} gates)")
        assert off <= gate and drift >= K.DRIFT_RATIO * gate
