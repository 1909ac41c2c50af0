"""hnet_filters with the keyframe track as an in-step measurement (include/hnet.h hnet_filters_set_keyframe_measure; csrc/kernels_filters_keyframe.hip;
DESIGN 7v).  A fleet that never heard of it, one that set and cleared it, the sessions next to measuring ones and sessions whose `when` keeps every
measurement out must agree byte for byte; per frame of a path with re-keys the in-step track must be hnet_sessions_keyframe_track's with the filter's own
step, the measurement and its innovation the host header's, the state the host twin's, and the keyframe store and map those of the same tracks made by
hand; FIRST, applied, LOST and GAP in one call each stay their session's alone; gates, a repeated attempt, advance and every refusal; the telescoping row.
4 to 8 sessions, max_batch 8, levels 3, 6 trials, paths of 9 frames (tests/keyframe_util.py)."""
import ctypes as C

import numpy as np
import pytest

import filters_keyframe_util as FK
import keyframe_util as KU
import test_gpu_filters as tg
import test_gpu_filters_innov as ti
import test_gpu_filters_photo_gate as pg
import test_gpu_filters_photo_refine as pr
import test_sessions_iterative_cpu as ic
from test_gpu_filters_photo_gate import _close_in_order  # noqa: F401  (autouse: closes what pg._track holds, the last one first)

pytestmark = pytest.mark.gpu

INVALID = 1
COUNTS = pg.COUNTS
T0 = 2.2                                   # tg._setup's twelve frames end at 2.1
K_HEAVY = 1e4           # every session weighs the network with 10 000 x the default k_net_cov: its updates apply and count, and hardly move the offsets, so
                        # that the step the track starts from is the state's own (the network of the test blob knows nothing of these frames)
EMPTY = np.zeros(0, np.dtype([("t", "<f8"), ("wm", "<f8", 3), ("am", "<f8", 3)]))
ZERO_STATS = {"asked": 0, "applied": 0, "unusable": 0, "nis_rejected": 0, "sum_nis": 0.0, "max_nis": 0.0}
# measured over every usable frame of test_path_with_rekeys: z_px and r_px, device against the host header on the device's record, and the innovation
# (r, s_diag, nis) against hnet_ekf::innovation on the host twin's posterior, relative as ti._rel: all 0 (the two sides share the code, the inverse is pinned
# by DESIGN 7l and no IMU interval lies between the states).  Gates: 10 x, which is equality
MEASURED_Z = MEASURED_RPX = MEASURED_INNOV = 0.0


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ti._build(tmp_path_factory.mktemp("filters_ref_kf"), "filters_ref")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return FK.build_ref(tmp_path_factory.mktemp("filters_keyframe_ref_gpu"))


def _mopts(**kw):
    _capi = tg._mods()[0]
    base = dict(levels=KU.LEVELS, max_iterations=KU.TRIALS, cov_scale=1.0)
    base.update(kw)
    return _capi.keyframe_measure_opts(**base)


def _track_kw(o):
    """the keyword form of o.track for HnetSessions.keyframe_track"""
    return KU.opts_kw(o.track)


def _seq_frames(seed=1):
    return KU.sequence("out-and-back", seed)[0]


def _slots(f, s, ids, got, sel, refine=False):
    """everything a step leaves, per listed slot of `sel`"""
    n = len(ids)
    pri, ph, inn, st = f.last_priors(n), f.last_photometric(n), f.last_innovations(n), f.get_state(ids)
    out = [(got[0][k].tobytes(), got[1][:, k].tobytes(), int(got[2][k]), pri[:, k].tobytes(), st[k].tobytes(), ph[k].tobytes(), inn[:, k].tobytes(), s.seq(int(ids[k])))
           for k in sel]
    if refine:
        out.append(f.last_refine(n).tobytes())
    return out


# ---- 1: never heard of it ------------------------------------------------------------------------------------------------------------------------------

def _heavy(ps, filters):
    for i, p in enumerate(ps):
        p.k_net_cov *= K_HEAVY
        for f in filters:
            f.set_params(i, p)


def _configure(s, f, mode, first):
    """the fleet under test; first: before its first call"""
    if not first:
        return
    s.enable_keyframes()
    if mode == "cleared":
        for i in range(8):
            f.set_keyframe_measure(i, _mopts())
        for i in range(8):
            f.set_keyframe_measure(i, None)
    elif mode == "others":
        for i in range(4):
            f.set_keyframe_measure(i, _mopts(cov_scale=1.0 + i))
    elif mode == "if_none":
        for i in range(8):
            f.set_keyframe_measure(i, _mopts(when=FK.IF_NONE))


def _check_mode(f, mode, n, tick, never_state, state):
    _capi = tg._mods()[0]
    if mode == "cleared":
        assert _capi.lib().hnet_filters_last_keyframe_measure(f._f, n, np.zeros(n, FK.MEASURE).ctypes.data) == INVALID
        return
    rr = f.last_keyframe_measure(n)
    print(f"{mode}, tick {tick}: flags {[hex(int(x)) for x in rr['flags']]}, track flags {[hex(int(x)) for x in rr['track']['flags']]}")
    if mode == "others":
        assert rr[4:].tobytes() == np.zeros(n - 4, FK.MEASURE).tobytes() and np.all(rr["flags"][:4] & FK.ASKED)
        if tick == 0:
            assert all(int(x) == FK.ASKED | FK.FIRST for x in rr["flags"][:4])
        else:
            applied = [k for k in range(4) if rr["flags"][k] & FK.APPLIED]
            # (a session without an IMU interval has zero offset covariance behind the last reset: its gain is zero and the measurement moves nothing)
            moving = [k for k in applied if COUNTS[k] > 0]
            print("  moved [m]:", [float(np.abs(state["p"][k] - never_state["p"][k]).max()) for k in range(4)], "NIS", np.round(rr["innov"]["nis"][:4], 1).tolist())
            assert moving, "no measuring session applied its measurement: the test shows nothing"
            assert all(state[k].tobytes() != never_state[k].tobytes() for k in moving)
    else:
        want = FK.ASKED | FK.NOT_SELECTED
        assert all(int(x) & ~FK.UNUSABLE == want for x in rr["flags"]) and not np.any(rr["flags"] & FK.APPLIED)
        assert all(f.keyframe_measure_stats(i)["applied"] == 0 and f.keyframe_measure_stats(i)["asked"] == tick + 1 for i in range(8))


@pytest.mark.parametrize("mode", ["cleared", "others", "if_none"])
@pytest.mark.parametrize("iters", [1, 3])
def test_never_heard_of_it_step(blob, iters, mode):
    """two steps (the second on a frame the first one's keyframe aligns with) of a fleet without the API against one that set and cleared the feature on all
    8 sessions (and both with an idle photometric fallback: the refine records too), one where only sessions 0 .. 3 measure (sessions 4 .. 7 compared:
    their last update ran with update_offset = 1 and left the reset to the measurement's launch; a measuring neighbour is applied) and one where all 8
    measure under IF_NONE while every update applies: states, outputs, priors, updates, sequence numbers, innovation and photometric records byte-equal"""
    _capi, _, _, HnetFilters = tg._mods()
    ea, sa, fa = pg._fleet(blob, iters, True)
    eb, sb, fb = pg._fleet(blob, iters, True)
    ids = np.arange(8, dtype=np.int32)
    sel = range(4, 8) if mode == "others" else range(8)
    frames = _seq_frames()
    ps, sts, imus = ti._inputs(_capi, HnetFilters, 90 + iters, 8, T0, COUNTS)
    for p in ps:
        p.k_net_cov *= K_HEAVY
    rng = np.random.default_rng(7)
    t2 = [T0 + 0.002 * max(COUNTS[i], 1) + 0.0004 for i in range(8)]
    imus2 = [tg._imu(rng, T0 + ps[i].cam_imu_dt, COUNTS[i]) for i in range(8)]
    for f, s in ((fa, sa), (fb, sb)):
        ti._load(f, s, ps, sts, seq=7)
        for i in range(8):
            f.set_photo_gate(i, 1e30)
    _configure(sb, fb, mode, True)
    if mode == "cleared":
        for f in (fa, fb):
            for i in range(8):
                f.set_photo_refine(i, pr._ropts())
    for tick, (t, im, fr) in enumerate((([T0] * 8, imus, frames[0]), (t2, imus2, frames[1]))):
        for s in (sa, sb):
            s.push(ids, np.repeat(fr[None], 8, 0), t=list(t))
        a, b = fa.step(ids, t, im), fb.step(ids, t, im)
        assert _slots(fa, sa, ids, a, sel, mode == "cleared") == _slots(fb, sb, ids, b, sel, mode == "cleared"), tick
        assert list(a[2]) == [iters] * 8
        _check_mode(fb, mode, 8, tick, a[0], b[0])
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


@pytest.mark.parametrize("mode", ["cleared", "others", "if_none"])
@pytest.mark.parametrize("iters", [1, 3])
def test_never_heard_of_it_advance(blob, iters, mode):
    """the same for three hnet_filters_advance ticks on rings of 64 readings that wrap"""
    _capi = tg._mods()[0]
    ea, sa, fa = pg._fleet(blob, iters, True)
    eb, sb, fb = pg._fleet(blob, iters, True)
    ps, _, hist, t_frame = pr._advance_rig([(sa, fa), (sb, fb)], 23, 1e30, 3 * 42 + 4)
    _heavy(ps, (fa, fb))
    _configure(sb, fb, mode, True)
    ids = np.arange(8, dtype=np.int32)
    sel = range(4, 8) if mode == "others" else range(8)
    fed = [0] * 8
    frames = _seq_frames()
    for tick in range(3):
        t_frame = t_frame + 0.002 * np.maximum(COUNTS, 0.1) + 0.0004
        for s in (sa, sb):
            s.push(ids, np.repeat(frames[tick][None], 8, 0), t=list(t_frame))
        chunks = pr._chunks(hist, ps, t_frame, fed)
        for f in (fa, fb):
            f.feed_imu(ids, chunks)
        a, b = fa.advance(ids), fb.advance(ids)
        assert list(b[3]) == [_capi.ADV_STEPPED] * 8 and list(a[2]) == [iters] * 8
        assert _slots(fa, sa, ids, a[:3], sel) == _slots(fb, sb, ids, b[:3], sel), tick
        _check_mode(fb, mode, 8, tick, a[0], b[0])
    assert max(fed) > 64
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


# ---- the rig of the path tests -----------------------------------------------------------------------------------------------------------------------------

def _rig(blob, iters, n, map_capacity=0, innov=True, seed=3, k_net_cov=None):
    """n sessions behind tg._setup's twelve frames (the reference gate is open), keyframes (and a map) enabled, parameters set"""
    _capi, _, _, HnetFilters = tg._mods()
    e, s, f = pg._track(*tg._setup(blob, n, iters))
    if innov:
        f.enable_innovations()
    s.enable_keyframes()
    if map_capacity:
        s.enable_keyframe_map(map_capacity)
    rng = np.random.default_rng(seed)
    ps = [tg._params(HnetFilters, rng, i) for i in range(n)]
    for i, p in enumerate(ps):
        p.k_net_cov = p.k_net_cov * K_HEAVY if k_net_cov is None else k_net_cov
        f.set_params(i, p)
    return (e, s, f), ps, rng


def _state_with_step(rng, step_px, t):
    """a filter state at time t whose (x, y) offsets are step_px / 159.5"""
    _capi = tg._mods()[0]
    st = tg._state(_capi, rng, t)
    st["offset"][0][:, :2] = np.asarray(step_px, np.float64).reshape(4, 2) / FK.F
    return st


def _tick(s, f, ids, frames, t, states):
    """the sessions ids get their frame at time t and their state (just before t), and step without an IMU interval"""
    n = len(ids)
    s.push(ids, np.stack(frames), t=[t] * n)
    for k, i in enumerate(ids):
        f.set_state(int(i), states[k])
    return f.step(ids, [t] * n, [EMPTY] * n)


def _want_stats(recs):
    st = dict(ZERO_STATS)
    for r in recs:
        fl = int(r["flags"])
        if not fl & FK.ASKED:
            continue
        st["asked"] += 1
        st["applied"] += int(bool(fl & FK.APPLIED))
        st["unusable"] += int(bool(fl & FK.UNUSABLE))
        st["nis_rejected"] += int(bool(fl & FK.NIS_REJECTED))
        if fl & (FK.APPLIED | FK.NIS_REJECTED) and np.isfinite(r["innov"]["nis"]):
            st["sum_nis"] += float(r["innov"]["nis"])
            st["max_nis"] = max(st["max_nis"], float(r["innov"]["nis"]))
    return st


def _check_stats(f, ids, calls):
    keys = ("asked", "applied", "unusable", "nis_rejected", "max_nis")
    for k, i in enumerate(ids):
        want, got = _want_stats([rr[k] for rr in calls]), f.keyframe_measure_stats(int(i))
        assert {x: got[x] for x in keys} == {x: want[x] for x in keys}, (i, got, want)
        assert got["sum_nis"] == pytest.approx(want["sum_nis"], rel=1e-12, abs=0.0)
        f.reset_keyframe_measure_stats(int(i))
        assert f.keyframe_measure_stats(int(i)) == ZERO_STATS


# ---- 2: per frame of a path with re-keys ---------------------------------------------------------------------------------------------------------------------

def test_path_with_rekeys(blob, ref, lib):
    """the out-and-back path of seeds 1, 2, 5, 11 (one session each), max_age = 3 (re-keys at frames 3 and 6), a map of 3 slots, 3 iterations whose updates
    all apply, the state's offsets at the noisy steps.  Per frame and session: start_px = compose(step_px, key_px before) bit for bit by the host header;
    track.rec = hnet_op_photo_align_robust(keyframe, curr, start_px) byte for byte; the rest of track = the host header's decide byte for byte; z_px, r_px
    and the innovation = the host header's on the device's record (relative difference 0); step_px within one fp32 ulp of the host twin's and the state
    within 1e-10 of it; the keyframe, the map and the records equal those of a second sessions object tracked by hand with the same steps, and a plain
    hnet_sessions_keyframe_track that follows behaves the same on both"""
    _capi, HnetEngine, HnetSessions, _ = tg._mods()
    seeds, n, iters = FK.ROW_SEEDS, 4, 3
    (e, s, f), ps, rng = _rig(blob, iters, n, map_capacity=3)
    e2, s2, _f2 = pg._track(*tg._setup(blob, n, 1))                           # the hand-tracked twin: sessions only
    s2.enable_keyframes()
    s2.enable_keyframe_map(3)
    kref = C.CDLL(lib._name)
    ids = np.arange(n, dtype=np.int32)
    o = _mopts(cov_scale=2.0, max_age=3)
    for i in ids:
        f.set_keyframe_measure(int(i), o)
    seqs = [KU.sequence("out-and-back", sd) for sd in seeds]
    host = [FK.new_session() for _ in range(n)]                               # key state by the host header's decide, prev_ok by its rule
    worst = dict(z=0.0, r_px=0.0, innov=0.0, ulp=0.0)
    calls, applied = [], 0
    for fi in range(9):
        t = T0 + 0.1 * fi
        frames = [seqs[k][0][fi] for k in range(n)]
        states = [_state_with_step(rng, seqs[k][2][fi], t - 0.05) for k in range(n)]
        keys_before = [s2.keyframe(int(i)) if host[k]["key"]["has_key"][0] else None for k, i in enumerate(ids)]
        out, net, upd = _tick(s, f, ids, frames, t, states)
        rr = f.last_keyframe_measure(n)
        calls.append(rr)
        s2.push(ids, np.stack(frames), t=[t] * n)
        hand = s2.keyframe_track(ids, step_px=rr["step_px"], **_track_kw(o))
        assert hand.tobytes() == rr["track"].tobytes(), fi                    # the in-step track is the call made by hand with the filter's own step
        print(f"frame {fi}: flags {[hex(int(x)) for x in rr['flags']]}, track flags {[hex(int(x)) for x in rr['track']['flags']]}, updates {list(upd)}")
        for k, i in enumerate(ids):
            r, hs = rr[k], host[k]
            had_key, key_prev, prev_ok = bool(hs["key"]["has_key"][0]), hs["key"]["key_px"][0].copy(), int(hs["prev_ok"][0])
            accepted = 0
            if had_key:
                start = KU.ref_compose(kref, r["step_px"], key_prev)
                assert start is not None and r["track"]["start_px"].tobytes() == start.tobytes(), (fi, k)
                op, lv = e.op_photo_align_robust(keys_before[k], frames[k], start, levels=KU.LEVELS, want_levels=True, max_iterations=KU.TRIALS)
                assert r["track"]["rec"].tobytes() == op[0].tobytes(), (fi, k)
                accepted = int(lv[0]["px"]["accepted"].sum())
            ns, dout, copy = KU.ref_decide(kref, hs["key"], r["track"]["start_px"], r["track"]["rec"], o.track, False)
            assert dout[0].tobytes() == r["track"].tobytes(), (fi, k)           # decide: every byte of the record
            ok, z, r_px, m72, fl = FK.ref_measure(lib, had_key, key_prev, prev_ok, r["track"], accepted, o, ps[k].k_net_cov)
            assert int(r["flags"]) & FK.UNUSABLE == fl and r["pad"] == 0, (fi, k, hex(int(r["flags"])), hex(fl))
            # the host twin: propagation without an interval, the step's own outputs, the device's record as the aligner's
            st = np.array(states[k], dtype=_capi.FILTER_STATE_DTYPE).reshape(1).copy()
            assert ref.ref_propagate_with_imu(C.c_void_p(st.ctypes.data), C.byref(ps[k]), C.c_double(t), C.c_void_p(EMPTY.ctypes.data), 0) >= 0
            tw = FK.ref_iterated(lib, st, ps[k], net[:, k, :], 1, 0.0, np.zeros(1 + iters, FK.PHOTO), 0.0, o, False, hs, align_rec=r["track"]["rec"], accepted=accepted)
            ulp = np.abs(r["step_px"].astype(np.float64) - tw["rec"]["step_px"].astype(np.float64)) / np.spacing(np.abs(tw["rec"]["step_px"]))
            worst["ulp"] = max(worst["ulp"], float(ulp.max()))
            assert ulp.max() <= 1.0, (fi, k, ulp)
            assert tw["rec"]["flags"] == r["flags"] and tw["updates"] == upd[k], (fi, k, hex(int(tw["rec"]["flags"])), hex(int(r["flags"])))
            tg._close(out[k], tw["state"][0])
            if ok:
                assert r["flags"] == FK.ASKED | FK.APPLIED and upd[k] == iters + 1
                worst["z"] = max(worst["z"], ti._rel(r["z_px"], z))
                worst["r_px"] = max(worst["r_px"], float(np.abs(r["r_px"] - r_px).max() / np.abs(r_px).max()))
                worst["innov"] = max(worst["innov"], max(ti._rel(r["innov"][fld], tw["rec"]["innov"][fld]) for fld in ("r", "s_diag", "nis")))
                assert r["innov"]["flag"] == FK.INN_USED and r["innov"]["iteration"] == iters
                applied += 1
            else:
                assert not r["z_px"].any() and not r["r_px"].any() and r["innov"]["flag"] == FK.INN_NONE and upd[k] == iters
            hs["key"], hs["prev_ok"] = ns, 0 if r["track"]["flags"] & _capi.KF_LOST else 1
            # the store and the map: those of the tracks made by hand
            assert s.keyframe(int(i)).tobytes() == s2.keyframe(int(i)).tobytes(), (fi, k)
            ea_, ma_ = s.keyframe_map_info(int(i))
            eb_, mb_ = s2.keyframe_map_info(int(i))
            assert ea_.tobytes() == eb_.tobytes() and ma_.tobytes() == mb_.tobytes(), (fi, k)
            for slot in range(3):
                if ea_["valid"][slot]:
                    assert s.map_keyframe(int(i), slot).tobytes() == s2.map_keyframe(int(i), slot).tobytes(), (fi, k, slot)
        if fi in (3, 6):
            assert np.all(rr["track"]["flags"] & _capi.KF_MAX_AGE) and np.all(rr["track"]["flags"] & _capi.KF_REKEYED)
    print(f"worst: z rel {worst['z']:.2e}, r_px rel {worst['r_px']:.2e}, innovation rel {worst['innov']:.2e}, step_px {worst['ulp']:.2f} ulp; {applied} applied")
    assert applied >= 4 * 7
    assert worst["z"] <= 10 * MEASURED_Z and worst["r_px"] <= 10 * MEASURED_RPX and worst["innov"] <= 10 * MEASURED_INNOV
    _check_stats(f, ids, calls)
    # a plain track that follows: the same record on both, and no GAP (the mirrors of the keyframe layer saw the in-step tracks)
    extra = [seqs[k][0][7] for k in range(n)]
    for ss in (s, s2):
        ss.push(ids, np.stack(extra), t=[T0 + 1.0] * n)
    a, b = s.keyframe_track(ids, **_track_kw(o)), s2.keyframe_track(ids, **_track_kw(o))
    assert a.tobytes() == b.tobytes() and not np.any(a["flags"] & _capi.KF_GAP)
    for x in (f, _f2, s, s2, e, e2):
        x.close()


# ---- 3: the mixed call ---------------------------------------------------------------------------------------------------------------------------------------

def test_mixed_call(blob):
    """one call of four slots, out of order, auto_rekey off: session 5 FIRST, 2 TRACKED and applied, 7 LOST on a constant frame (bridged, the keyframe
    stays), 0 with GAP (a frame no track saw).  Each slot's record and state are those of a twin fleet that steps the sessions ONE PER CALL.  The next
    frame of session 7 tracks again and is PREV_NOT_MEASURED (the key_px before it was a bridge, not a measurement); the one after it is applied"""
    _capi = tg._mods()[0]
    frames = _seq_frames()
    steps = KU.sequence("out-and-back", 1)[2]
    const = np.full((224, 320), 93, np.uint8)
    rigs = [_rig(blob, 3, 8) for _ in range(2)]
    o = _mopts(cov_scale=2.0, auto_rekey=0)
    rng_states = np.random.default_rng(11)
    order = np.array([5, 2, 7, 0], np.int32)
    st0 = {int(i): _state_with_step(rng_states, np.zeros(8), T0 - 0.05) for i in (0, 2, 7)}
    st1 = {int(i): _state_with_step(rng_states, steps[1], T0 + 0.07) for i in order}
    st2 = _state_with_step(rng_states, np.zeros(8), T0 + 0.15)
    st3 = _state_with_step(rng_states, steps[2], T0 + 0.25)
    results = []
    for which, ((e, s, f), ps, _) in enumerate(rigs):
        for i in range(8):
            f.set_keyframe_measure(i, o)
        first = np.array([0, 2, 7], np.int32)
        groups = [first] if which == 0 else [np.array([i], np.int32) for i in first]
        for g in groups:                                                       # frame 0: sessions 0, 2, 7 take their keyframes
            _tick(s, f, g, [frames[0]] * len(g), T0, [st0[int(i)] for i in g])
            assert all(int(x) == FK.ASKED | FK.FIRST for x in f.last_keyframe_measure(len(g))["flags"])
        s.push(np.array([0], np.int32), frames[1][None], t=[T0 + 0.05])         # session 0: a frame no track sees
        cur = {5: frames[1], 2: frames[1], 7: const, 0: frames[1]}
        groups = [order] if which == 0 else [np.array([i], np.int32) for i in order]
        got = {}
        for g in groups:
            out, net, upd = _tick(s, f, g, [cur[int(i)] for i in g], T0 + 0.1, [st1[int(i)] for i in g])
            rr = f.last_keyframe_measure(len(g))
            for k, i in enumerate(g):
                got[int(i)] = (rr[k].tobytes(), out[k].tobytes(), int(upd[k]), int(rr["flags"][k]), int(rr["track"]["flags"][k]))
        results.append(got)
        if which == 0:
            print({i: (hex(v[3]), hex(v[4]), v[2]) for i, v in got.items()})
            assert got[5][3] == FK.ASKED | FK.FIRST and got[5][4] & _capi.KF_FIRST and got[5][2] == 3
            assert got[2][3] == FK.ASKED | FK.APPLIED and got[2][2] == 4
            assert got[7][3] == FK.ASKED | FK.TRACK_LOST and got[7][4] & _capi.KF_STOPPED and not got[7][4] & _capi.KF_REKEYED and got[7][2] == 3
            assert got[0][3] == FK.ASKED | FK.TRACK_GAP and got[0][4] & _capi.KF_GAP and got[0][2] == 3
            seven = np.array([7], np.int32)
            _, _, upd = _tick(s, f, seven, [frames[1]], T0 + 0.2, [st2])
            r = f.last_keyframe_measure(1)[0]
            assert r["flags"] == FK.ASKED | FK.PREV_NOT_MEASURED and not r["track"]["flags"] & _capi.KF_LOST and upd[0] == 3, (hex(int(r["flags"])), hex(int(r["track"]["flags"])))
            _, _, upd = _tick(s, f, seven, [frames[2]], T0 + 0.3, [st3])
            r = f.last_keyframe_measure(1)[0]
            assert r["flags"] == FK.ASKED | FK.APPLIED and upd[0] == 4, hex(int(r["flags"]))
            assert f.keyframe_measure_stats(7) == _want_stats_of(f, 7, 4)
    assert results[0] == results[1]
    for (e, s, f), _, _ in rigs:
        for x in (f, s, e):
            x.close()


def _want_stats_of(f, i, asked):
    """the counters of a session whose last record was applied, after `asked` measuring calls of which one was applied"""
    got = f.keyframe_measure_stats(i)
    assert got["asked"] == asked and got["applied"] == 1 and got["unusable"] == asked - 1 and got["nis_rejected"] == 0 and got["sum_nis"] == got["max_nis"] > 0.0
    return got


# ---- 4: the rest -----------------------------------------------------------------------------------------------------------------------------------------------

def test_gates(blob):
    """sessions 0 .. 3 on the second frame of the path: 0 applied; 1 with max_nis = 1e-30 is NIS_REJECTED and 2 with the measurement's max_mse = 1e-30
    UNUSABLE (MSE_ABOVE_MAX), each with the state of a fleet that measures nothing under the same gates, byte for byte; 3 does not measure"""
    frames = _seq_frames()
    rigs = [_rig(blob, 3, 4) for _ in range(2)]
    ids = np.arange(4, dtype=np.int32)
    rng = np.random.default_rng(5)
    sts = [[_state_with_step(rng, np.zeros(8), T0 + 0.1 * k - 0.05) for _ in range(4)] for k in range(2)]
    outs = []
    for which, ((e, s, f), ps, _) in enumerate(rigs):
        f.set_nis_gate(1, 1e-30)
        if which == 0:
            f.set_keyframe_measure(0, _mopts(cov_scale=2.0))
            f.set_keyframe_measure(1, _mopts(cov_scale=2.0))
            f.set_keyframe_measure(2, _mopts(cov_scale=2.0, max_mse=1e-30))
        for k in range(2):
            out, net, upd = _tick(s, f, ids, [frames[k]] * 4, T0 + 0.1 * k, sts[k])
        outs.append((out, upd))
        if which == 0:
            rr = f.last_keyframe_measure(4)
            print([hex(int(x)) for x in rr["flags"]], list(upd))
            assert rr["flags"][0] == FK.ASKED | FK.APPLIED and upd[0] == 4
            assert rr["flags"][1] == FK.ASKED | FK.NIS_REJECTED and rr["innov"]["flag"][1] == FK.INN_REJECTED and rr["innov"]["nis"][1] > 1e-30 and upd[1] == 0
            assert rr["flags"][2] == FK.ASKED | FK.MSE_ABOVE_MAX and not rr["r_px"][2].any() and not rr["z_px"][2].any() and upd[2] == 3
            assert rr[3].tobytes() == np.zeros(1, FK.MEASURE).tobytes() and upd[3] == 3
            assert f.innovation_stats(1)["rejected"] == 2                       # (the network's iteration 0 of both frames; the measurement's is its own statistic)
            assert f.keyframe_measure_stats(1)["nis_rejected"] == 1
    (out_a, upd_a), (out_b, upd_b) = outs
    assert out_a[0].tobytes() != out_b[0].tobytes()
    for k in (1, 2, 3):
        assert out_a[k].tobytes() == out_b[k].tobytes() and upd_a[k] == upd_b[k], k
    for (e, s, f), _, _ in rigs:
        for x in (f, s, e):
            x.close()


def test_repeat_counts_once(blob):
    """the overflowing iterative model of test_gpu_filters_photo_refine.test_repeat_counts_once with every session measuring, a map of 3 slots: the first
    step demotes the model once and repeats the attempt, the FIRST track and its commits with it; two frames on, records, states, keyframes, map and
    statistics are those of fresh objects whose iterative engine runs HNET_PREC_BF16X3 from the start - every track committed once"""
    from cuahn_vio_amd.homography_net import HnetEngine
    _capi, _, _, HnetFilters = tg._mods()
    iters, n = 3, 4
    ov = ic.overflow_iterative_blob()
    frames = _seq_frames()
    ids = np.arange(n, dtype=np.int32)
    rng0 = np.random.default_rng(47)
    ps = [tg._params(HnetFilters, rng0, i) for i in range(n)]
    for p in ps:
        p.k_net_cov *= K_HEAVY
    sts = [[_state_with_step(rng0, np.zeros(8), T0 + 0.1 * k - 0.05) for _ in range(n)] for k in range(3)]
    res = []
    for prec in (pg.PREC_F16X2, pg.PREC_BF16X3):
        e, s, f = tg._setup(blob, n, iters, precision=pg.PREC_F16X2)
        ie = HnetEngine(ov, variant="prior1", mc_samples=8, dropout_p=0.1, mc_seed=9, max_batch=8, precision=prec)
        pg._track(e, ie, s, f)
        s.set_iterative_model(ie)
        s.enable_keyframes()
        s.enable_keyframe_map(3)
        for i in ids:
            f.set_params(int(i), ps[i])
            f.set_keyframe_measure(int(i), _mopts(cov_scale=2.0, max_age=2))
        calls, outs = [], []
        for k in range(3):
            out, net, upd = _tick(s, f, ids, [frames[k]] * n, T0 + 0.1 * k, sts[k])
            if k == 0:
                assert ie.precision() == pg.PREC_BF16X3 and e.precision() == pg.PREC_F16X2      # (demoted once, the iterative context only)
            calls.append(f.last_keyframe_measure(n))
            outs.append((out.tobytes(), net.tobytes(), upd.tobytes()))
            assert np.all(np.isfinite(net))
        print([[hex(int(x)) for x in c["flags"]] for c in calls])
        assert np.all(calls[0]["flags"] == FK.ASKED | FK.FIRST) and np.all(calls[2]["track"]["flags"] & _capi.KF_REKEYED)
        keys = [s.keyframe(int(i)).tobytes() for i in ids]
        maps = [tuple(x.tobytes() for x in s.keyframe_map_info(int(i))) for i in ids]
        assert all(s.keyframe_map_info(int(i))[1]["serial"][0] == 2 for i in ids)      # two keyframes stored: the FIRST one once
        stats = [f.keyframe_measure_stats(int(i)) for i in ids]
        assert all(st["asked"] == 3 for st in stats) and [s.seq(int(i)) for i in ids] == [3 * iters] * n
        _check_stats(f, ids, calls)
        res.append((outs, [c.tobytes() for c in calls], keys, maps, stats))
        for o in (f, s, ie, e):
            o.close()
    assert res[0] == res[1]


def test_advance_equals_step(blob):
    """three hnet_filters_advance ticks on rings that wrap, every session measuring (max_age = 2: a re-key inside): states, outputs, updates, every kind of
    record, the measure records and statistics, keyframes and maps are those of hnet_filters_step calls with the windows taken from the full history"""
    _capi = tg._mods()[0]
    iters = 3
    ea, sa, fa = pg._fleet(blob, iters, True)
    eb, sb, fb = pg._fleet(blob, iters, True)
    ps, _, hist, t_frame = pr._advance_rig([(sa, fa), (sb, fb)], 29, 1e30, 3 * 42 + 4)
    _heavy(ps, (fa, fb))
    ids = np.arange(8, dtype=np.int32)
    for s, f in ((sa, fa), (sb, fb)):
        s.enable_keyframes()
        s.enable_keyframe_map(2)
        for i in range(8):
            f.set_keyframe_measure(i, _mopts(cov_scale=2.0, max_age=2, when=FK.IF_NONE if i == 3 else FK.ALWAYS))
    frames = _seq_frames()
    fed, calls = [0] * 8, []
    for tick in range(3):
        t_frame = t_frame + 0.002 * np.maximum(COUNTS, 0.1) + 0.0004
        for s in (sa, sb):
            s.push(ids, np.repeat(frames[tick][None], 8, 0), t=list(t_frame))
        fa.feed_imu(ids, pr._chunks(hist, ps, t_frame, fed))
        a = fa.advance(ids)
        b = fb.step(ids, list(t_frame), [hist[i][:fed[i]] for i in range(8)])
        assert list(a[3]) == [_capi.ADV_STEPPED] * 8
        assert pg._everything(fa, sa, ids, a[:3], True) == pg._everything(fb, sb, ids, b, True), tick
        ra, rb = fa.last_keyframe_measure(8), fb.last_keyframe_measure(8)
        assert ra.tobytes() == rb.tobytes() and np.all(ra["flags"] & FK.ASKED), tick
        assert all(int(a[2][i]) == iters + (1 if ra["flags"][i] & FK.APPLIED else 0) for i in range(8))
        print(f"tick {tick}: flags {[hex(int(x)) for x in ra['flags']]}")
        calls.append(ra)
        for i in range(8):
            assert sa.keyframe(i).tobytes() == sb.keyframe(i).tobytes()
            assert [x.tobytes() for x in sa.keyframe_map_info(i)] == [x.tobytes() for x in sb.keyframe_map_info(i)]
    assert np.any(calls[1]["flags"] & FK.APPLIED) and calls[1]["flags"][3] & FK.NOT_SELECTED and max(fed) > 64
    for f in (fa, fb):
        _check_stats(f, ids, calls)
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


def test_refusals_change_nothing(blob):
    """every HNET_ERR_INVALID_ARG of set_keyframe_measure, the accessors, and a step or advance whose measuring sessions differ in the track's options or
    step next to refining ones: nothing changed - the step that follows is the one of a fleet that never heard of the feature"""
    _capi, _, _, HnetFilters = tg._mods()
    ea, sa, fa = pg._fleet(blob, 1, True)
    eb, sb, fb = pg._fleet(blob, 1, True)
    L = _capi.lib()
    st = _capi.KeyframeMeasureStats()
    good = _mopts()
    buf = np.zeros(8, FK.MEASURE)
    assert L.hnet_filters_set_keyframe_measure(fa._f, 0, C.byref(good)) == INVALID               # before hnet_sessions_enable_keyframes
    sa.enable_keyframes()
    assert L.hnet_filters_keyframe_measure_stats(fa._f, 0, C.byref(st)) == INVALID and L.hnet_filters_reset_keyframe_measure_stats(fa._f, 0) == INVALID
    assert L.hnet_filters_last_keyframe_measure(fa._f, 8, buf.ctypes.data) == INVALID
    for bad_id in (-1, 8):
        assert L.hnet_filters_set_keyframe_measure(fa._f, bad_id, C.byref(good)) == INVALID
        assert L.hnet_filters_set_keyframe_measure(fa._f, bad_id, None) == INVALID
    assert L.hnet_filters_set_keyframe_measure(fa._f, 0, C.byref(_capi.keyframe_measure_opts())) == INVALID      # the defaults: cov_scale = 0
    for kw in (dict(levels=0), dict(levels=5), dict(cov_scale=-1.0), dict(cov_scale=float("nan")), dict(cov_scale=float("inf")), dict(sigma_floor_px=-0.1),
               dict(sigma_floor_px=float("nan")), dict(max_mse=-1.0), dict(max_mse=float("inf")), dict(when=2), dict(when=-1), dict(huber_k=-1.0),
               dict(max_iterations=33), dict(brightness=2), dict(auto_rekey=2), dict(max_age=-1), dict(rekey_overlap=1.5), dict(track_max_mse=-1.0)):
        assert L.hnet_filters_set_keyframe_measure(fa._f, 0, C.byref(_mopts(**kw))) == INVALID, kw
    fa.set_keyframe_measure(5, None)                                            # off before it was ever on: accepted, and nothing is allocated
    assert L.hnet_filters_keyframe_measure_stats(fa._f, 5, C.byref(st)) == INVALID
    # a session cannot have both: either order is refused
    fa.set_photo_refine(1, pr._ropts())
    assert L.hnet_filters_set_keyframe_measure(fa._f, 1, C.byref(good)) == INVALID
    fa.set_keyframe_measure(2, _mopts(levels=2))
    assert L.hnet_filters_set_photo_refine(fa._f, 2, C.byref(pr._ropts())) == INVALID
    fa.set_keyframe_measure(6, _mopts(levels=3))
    assert L.hnet_filters_keyframe_measure_stats(fa._f, 8, C.byref(st)) == INVALID and L.hnet_filters_reset_keyframe_measure_stats(fa._f, -1) == INVALID
    ps, sts, imus = ti._inputs(_capi, HnetFilters, 61, 8, pg.T_FRAME, COUNTS)
    ids = np.arange(8, dtype=np.int32)
    for f, s in ((fa, sa), (fb, sb)):
        ti._load(f, s, ps, sts, seq=7)
        for i in ids:
            f.set_photo_gate(int(i), 1e30)
    before = fa.get_state(ids).tobytes()

    def refused(sub):
        with pytest.raises(_capi.HnetError) as err:
            fa.step(sub, [pg.T_FRAME] * len(sub), [imus[int(i)] for i in sub])
        assert err.value.status == INVALID and fa.get_state(ids).tobytes() == before and [sa.seq(int(i)) for i in ids] == [7] * 8
    refused(ids)                                                                # 2 and 6 differ in levels
    refused(np.array([1, 2], np.int32))                                         # a refining and a measuring session in one call
    fa.set_keyframe_measure(6, _mopts(levels=2, max_age=4))
    refused(np.array([2, 6], np.int32))                                         # ... and in max_age
    fa.set_keyframe_measure(6, _mopts(levels=2, cov_scale=7.0, when=FK.IF_NONE))
    assert L.hnet_filters_last_keyframe_measure(fa._f, 8, buf.ctypes.data) == INVALID      # no call was accepted yet
    for i in (1, 2, 6):
        fa.set_photo_refine(i, None) if i == 1 else fa.set_keyframe_measure(i, None)
    a, b = fa.step(ids, [pg.T_FRAME] * 8, imus), fb.step(ids, [pg.T_FRAME] * 8, imus)
    assert pg._everything(fa, sa, ids, a, True) == pg._everything(fb, sb, ids, b, True) and list(a[2]) == [1] * 8
    assert L.hnet_filters_last_keyframe_measure(fa._f, 8, buf.ctypes.data) == INVALID      # the last call ran without a measuring session
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


def test_mismatch_is_refused_by_advance(blob):
    """hnet_filters_advance with two stepping sessions whose track options differ: HNET_ERR_INVALID_ARG, states, times and sequence numbers as they were;
    with the options made equal the same frame is then served"""
    _capi = tg._mods()[0]
    e, s, f = pg._fleet(blob, 1, False)
    ps, _, hist, t_frame = pr._advance_rig([(s, f)], 31, 1e30, 50)
    ids = np.arange(8, dtype=np.int32)
    s.enable_keyframes()
    f.set_keyframe_measure(2, _mopts(levels=2))
    f.set_keyframe_measure(6, _mopts(levels=3))
    t_frame = t_frame + 0.002 * np.maximum(COUNTS, 0.1) + 0.0004
    s.push(ids, np.repeat(_seq_frames()[0][None], 8, 0), t=list(t_frame))
    f.feed_imu(ids, pr._chunks(hist, ps, t_frame, [0] * 8))
    before, seqs = f.get_state(ids).tobytes(), [s.seq(int(i)) for i in ids]
    with pytest.raises(_capi.HnetError) as err:
        f.advance(ids)
    assert err.value.status == INVALID and f.get_state(ids).tobytes() == before and [s.seq(int(i)) for i in ids] == seqs
    with pytest.raises(_capi.HnetError):
        s.keyframe(2)                                                           # no keyframe was taken
    f.set_keyframe_measure(6, _mopts(levels=2))
    out, net, upd, status = f.advance(ids)
    rr = f.last_keyframe_measure(8)
    assert list(status) == [_capi.ADV_STEPPED] * 8 and list(upd) == [1] * 8
    assert [int(x) for x in rr["flags"]] == [FK.ASKED | FK.FIRST if i in (2, 6) else 0 for i in range(8)]
    for o in (f, s, e):
        o.close()


# ---- 5: the telescoping row on the device ------------------------------------------------------------------------------------------------------------------------

def test_telescoping_row_on_the_device(blob, lib):
    """tests/test_filters_keyframe_cpu.py::test_telescoping_row on the device: one session per seed, k_net_cov = 1e12 (the network's own updates carry no
    weight), the state's offsets at the noisy steps.  The running composition of H(z_px) stays within 7p's gate at every frame, the composed noisy steps end
    at least 3 gates off, and both figures equal the host row's to the printed digit (1e-4 px)"""
    n = 4
    (e, s, f), ps, rng = _rig(blob, 1, n, k_net_cov=1e12)
    ids = np.arange(n, dtype=np.int32)
    o = _mopts(rekey_overlap=KU.ROWS["out-and-back"][0])
    for i in ids:
        f.set_keyframe_measure(int(i), o)
    seqs = [KU.sequence("out-and-back", sd) for sd in FK.ROW_SEEDS]
    recs = []
    for fi in range(9):
        t = T0 + 0.1 * fi
        states = [FK.row_state(seqs[k][2][fi], t - 0.05) for k in range(n)]
        _tick(s, f, ids, [seqs[k][0][fi] for k in range(n)], t, states)
        recs.append(f.last_keyframe_measure(n))
    for k, seed in enumerate(FK.ROW_SEEDS):
        dev = np.stack([r[k] for r in recs])
        assert dev["flags"][0] == FK.ASKED | FK.FIRST and all(int(x) == FK.ASKED | FK.APPLIED for x in dev["flags"][1:]), [hex(int(x)) for x in dev["flags"]]
        worst, drift, per = FK.row_figures(dev, seed)
        hworst, hdrift, hper = FK.row_figures(FK.ref_row(lib, seed), seed)
        print(f"seed {seed}: device worst {worst:.4f} px (host {hworst:.4f}), per frame {np.round(per, 4).tolist()}; noisy steps {drift:.4f} px = {drift / FK.ROW_GATE:.2f} gates")
        assert worst <= FK.ROW_GATE and drift >= KU.DRIFT_RATIO * FK.ROW_GATE
        assert abs(worst - hworst) <= 1e-4 and abs(drift - hdrift) <= 1e-4 and np.abs(np.array(per) - np.array(hper)).max() <= 1e-4
    for x in (f, s, e):
        x.close()
