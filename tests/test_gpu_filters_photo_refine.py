"""hnet_filters with the photometric fallback (include/hnet.h hnet_filters_set_photo_refine; csrc/kernels_filters_refine.hip).  Off must be
off and a fallback nobody needs must change nothing, bit for bit; after a refusal at iteration 0 the refine record must be the record
hnet_sessions_photo_align_robust gives from the step's own prior, the measurement and its innovation the host header's, and the state the one
hnet_ekf::iterated_update_photo_refined leaves; the refined offsets must be near the truth; unusable, NIS-refused and switched-off fallbacks leave the
refusal's state and their neighbours alone; advance equals step; a repeated attempt counts once.  8 sessions, max_batch 8 (tests/test_gpu_filters.py
_setup), alignment options levels = 2, max_iterations = 3.  The frames of the tests with a refusal are photo_align_util.smooth_pair's, pushed behind
_setup's twelve, so that the alignment has a minimum."""
import ctypes as C

import numpy as np
import pytest

import photo_align_util as U
import test_gpu_filters as tg
import test_gpu_filters_innov as ti
import test_gpu_filters_photo_gate as pg
import test_sessions_iterative_cpu as ic
from test_gpu_filters_photo_gate import _close_in_order  # noqa: F401  (autouse: closes what pg._track holds, the last one first)

pytestmark = pytest.mark.gpu

INVALID = 1
ASKED, APPLIED, NIS_REJECTED, S_SINGULAR = 1, 2, 4, 8
STOPPED, NO_STEP, MSE_ABOVE_MAX = 32, 64, 128
UNUSABLE = 16 | 32 | 64 | 128 | 256 | 512
NONE, USED, REJECTED, SINGULAR, SKIPPED = range(5)
COUNTS = pg.COUNTS
T_PREV, T_FRAME = 1.0 + 0.1 * 12, 1.0 + 0.1 * 13                              # the smooth pair lies behind _setup's twelve frames
K_ALL = 1000.0          # every session weighs the network with 1000 x the default k_net_cov, so that the ratios of the unrefused hardly move (pg.K_LO)
# measured over the refused sessions of test_refusal_at_iteration_zero_composes: r_px, device against the host header on the same record, max |d - h| /
# max |h|, and the fallback's innovation (r, s_diag, nis) against hnet_ekf::innovation on the host-propagated state, relative as ti._rel: both 0 (equal, as
# expected of code the two sides share, with the inverse pinned by DESIGN 7l).  Gates: 10 x, which is equality
MEASURED_RPX, MEASURED_INNOV = 0.0, 0.0
ZERO_STATS = {"asked": 0, "applied": 0, "unusable": 0, "nis_rejected": 0, "sum_nis": 0.0, "max_nis": 0.0}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ti._build(tmp_path_factory.mktemp("filters_ref_pr"), "filters_ref")


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return ti._build(tmp_path_factory.mktemp("filters_photo_refine_ref_pr"), "filters_photo_refine_ref")


def _ropts(**kw):
    _capi = tg._mods()[0]
    base = dict(levels=2, max_iterations=3, cov_scale=1.0)
    base.update(kw)
    return _capi.photo_refine_opts(**base)


def _everything(f, s, ids, got, innov):
    return pg._everything(f, s, ids, got, innov)


def _push_pairs(s, seeds, curr=None):
    """the smooth pair of seeds[i] as session i's previous and current frame; curr: {session: frame} replaces a current frame"""
    ids = np.arange(len(seeds), dtype=np.int32)
    i1 = np.stack([U.smooth_pair(int(sd), 2.0)[0] for sd in seeds])
    i2 = np.stack([U.smooth_pair(int(sd), 2.0)[1] for sd in seeds])
    for k, fr in (curr or {}).items():
        i2[k] = fr
    s.push(ids, i1, t=[T_PREV] * len(seeds))
    s.push(ids, i2, t=[T_FRAME] * len(seeds))


def _inputs(seed, zero_offsets=False):
    _capi, _, _, HnetFilters = tg._mods()
    ps, sts, imus = ti._inputs(_capi, HnetFilters, seed, 8, T_FRAME, [0] if zero_offsets else COUNTS)    # (no IMU interval: the zero offsets stay zero)
    for p in ps:
        p.k_net_cov *= K_ALL
    if zero_offsets:
        for st in sts:
            st["offset"] = 0.0
    return ps, sts, imus


# ---- a, b: off is off; on, but nothing refused ------------------------------------------------------------------------------------------------------

def _configure(f, mode):
    for i in range(8):
        f.set_photo_gate(i, 1e30)
    if mode == "cleared":
        for i in range(8):
            f.set_photo_refine(i, _ropts())
        for i in range(8):
            f.set_photo_refine(i, None)
    elif mode == "on":
        for i in range(8):
            f.set_photo_refine(i, _ropts(cov_scale=1.0 + i))


def _check_idle(f, mode, n):
    _capi = tg._mods()[0]
    if mode == "on":
        rr = f.last_refine(n)
        assert rr.tobytes() == np.zeros(n, _capi.PHOTO_REFINE_DTYPE).tobytes()
        assert all(f.refine_stats(i) == ZERO_STATS for i in range(8))
    elif mode == "cleared":
        assert _capi.lib().hnet_filters_last_refine(f._f, n, np.zeros(n, _capi.PHOTO_REFINE_DTYPE).ctypes.data) == INVALID


@pytest.mark.parametrize("mode", ["cleared", "on"])
@pytest.mark.parametrize("iters", [1, 3])
def test_idle_changes_nothing_step(blob, iters, mode):
    """a. a fleet that never calls set_photo_refine against one that sets it on all 8 sessions and clears it again; b. against one that has it on under a
    gate of 1e30 (nothing refused: the last update runs with last = 0 and the fallback's update launch only resets): states, net_out, priors, updates,
    sequence numbers, photometric and innovation records are byte-equal; b. the refine records are zero and the statistics empty"""
    _capi, _, _, HnetFilters = tg._mods()
    ea, sa, fa = pg._fleet(blob, iters, True)
    eb, sb, fb = pg._fleet(blob, iters, True)
    _configure(fa, "never")
    _configure(fb, mode)
    ids = np.arange(8, dtype=np.int32)
    ps, sts, imus = ti._inputs(_capi, HnetFilters, 70 + iters, 8, pg.T_FRAME, COUNTS)
    for f, s in ((fa, sa), (fb, sb)):
        ti._load(f, s, ps, sts, seq=7)
    a, b = fa.step(ids, [pg.T_FRAME] * 8, imus), fb.step(ids, [pg.T_FRAME] * 8, imus)
    assert _everything(fa, sa, ids, a, True) == _everything(fb, sb, ids, b, True)
    assert list(b[2]) == [iters] * 8 and [sb.seq(int(i)) for i in ids] == [7 + iters] * 8
    assert np.all(b[0]["offset"] == 0) and np.all(b[0]["cov"][:, 15:, :] == 0)
    _check_idle(fb, mode, 8)
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


def _advance_rig(fleets, seed, gate, n_hist):
    """the set-up of pg.test_gate_that_cannot_reject_changes_nothing_advance on every fleet (s, f): rings of 64, one IMU stream per session"""
    _capi, _, _, HnetFilters = tg._mods()
    rng = np.random.default_rng(seed)
    t_frame = np.full(8, pg.T_FRAME)
    ps, sts, hist = [], [], []
    for s, f in fleets:
        f.enable_feed(64)
    for i in range(8):
        p = tg._params(HnetFilters, rng, i)
        st = tg._state(_capi, rng, t_frame[i])
        for s, f in fleets:
            f.set_params(i, p)
            f.set_state(i, st)
            f.set_photo_gate(i, gate)
        ps.append(p)
        sts.append(st)
        ts = t_frame[i] + p.cam_imu_dt - 0.0007 + 0.002 * np.arange(n_hist)
        r = np.zeros(len(ts), _capi.IMU_DTYPE)
        r["t"], r["wm"], r["am"] = ts, rng.standard_normal((len(ts), 3)) * 0.3, rng.standard_normal((len(ts), 3)) * 0.5 + [0, 0, 9.81]
        hist.append(r)
    return ps, sts, hist, t_frame


def _chunks(hist, ps, t_frame, fed):
    out = []
    for i in range(8):
        upto = int(np.searchsorted(hist[i]["t"], t_frame[i] + ps[i].cam_imu_dt, side="right")) + 1
        out.append(hist[i][fed[i]:upto])
        fed[i] = upto
    return out


@pytest.mark.parametrize("mode", ["cleared", "on"])
@pytest.mark.parametrize("iters", [1, 3])
def test_idle_changes_nothing_advance(blob, iters, mode):
    """a, b. the same for three hnet_filters_advance ticks on rings of 64 readings that wrap"""
    _capi = tg._mods()[0]
    ea, sa, fa = pg._fleet(blob, iters, True)
    eb, sb, fb = pg._fleet(blob, iters, True)
    ps, _, hist, t_frame = _advance_rig([(sa, fa), (sb, fb)], 23, 1e30, 3 * 42 + 4)
    _configure(fa, "never")
    _configure(fb, mode)
    ids = np.arange(8, dtype=np.int32)
    fed = [0] * 8
    fr = tg._frames(np.random.default_rng(5), 3)
    for tick in range(3):
        t_frame = t_frame + 0.002 * np.maximum(COUNTS, 0.1) + 0.0004
        for s in (sa, sb):
            s.push(ids, np.repeat(fr[tick][None], 8, 0), t=list(t_frame))
        chunks = _chunks(hist, ps, t_frame, fed)
        for f in (fa, fb):
            f.feed_imu(ids, chunks)
        a, b = fa.advance(ids), fb.advance(ids)
        assert list(b[3]) == [_capi.ADV_STEPPED] * 8 and list(b[2]) == [iters] * 8
        assert _everything(fa, sa, ids, a, True) == _everything(fb, sb, ids, b, True), tick
        _check_idle(fb, mode, 8)
    assert max(fed) > 64
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


# ---- c: the composition -------------------------------------------------------------------------------------------------------------------------------

def _ungated(blob, seeds, seed, iters=3, zero_offsets=False, seqs=None, curr=None):
    """a fleet with records on and the smooth pairs of `seeds` as its current pairs, the shared inputs and its ungated step"""
    e, s, f = pg._fleet(blob, iters, True)
    _push_pairs(s, seeds, curr)
    ps, sts, imus = _inputs(seed, zero_offsets)
    ids = np.arange(8, dtype=np.int32)
    seqs = [4] * 8 if seqs is None else seqs

    def load(f_=f, s_=s):
        ti._load(f_, s_, ps, sts)
        for i in range(8):
            s_.set_seq(i, seqs[i])
    load()
    ung = f.step(ids, [T_FRAME] * 8, imus)
    rec = f.last_photometric(8)
    assert list(ung[2]) == [iters] * 8 and not rec["flags"].any() and np.all(rec["n_inside"][:, 1:] >= 1)
    return (e, s, f), (ps, sts, imus), ids, ung, rec, pg._ratios(rec), load


def _midpoint_gate(ratio):
    order = np.sort(ratio[:, 0])[::-1]
    assert order[3] != order[4], order
    gate = 0.5 * (order[3] + order[4])
    above = ratio[:, 0] > gate
    print(f"iteration-0 ratios {np.array2string(ratio[:, 0], precision=5)}, gate {gate:.6g}; later {np.array2string(ratio[:, 1:].T, precision=5)}")
    assert above.sum() == 4
    assert ratio[~above].max() < gate, "the 4 below must stay below in the later iterations, or the rule refuses them there"
    return gate, above


def _want_stats(recs):
    """hnet_refine_stats of one session from its refine records of the accepted calls"""
    st = dict(ZERO_STATS)
    for r in recs:
        fl = int(r["flags"])
        if not fl & ASKED:
            continue
        st["asked"] += 1
        st["applied"] += int(bool(fl & APPLIED))
        st["unusable"] += int(bool(fl & UNUSABLE))
        st["nis_rejected"] += int(bool(fl & NIS_REJECTED))
        if fl & (APPLIED | NIS_REJECTED) and np.isfinite(r["innov"]["nis"]):
            st["sum_nis"] += float(r["innov"]["nis"])
            st["max_nis"] = max(st["max_nis"], float(r["innov"]["nis"]))
    return st


def _check_stats(f, ids, calls):
    for k, i in enumerate(ids):
        want = _want_stats([rr[k] for rr in calls])
        got = f.refine_stats(int(i))
        assert {key: got[key] for key in ("asked", "applied", "unusable", "nis_rejected", "max_nis")} == {key: want[key] for key in ("asked", "applied", "unusable", "nis_rejected", "max_nis")}, (i, got, want)
        assert got["sum_nis"] == pytest.approx(want["sum_nis"], rel=1e-12, abs=0.0)
        f.reset_refine_stats(int(i))
        assert f.refine_stats(int(i)) == ZERO_STATS


def _host_measure(rref, rec, accepted, o, k):
    _capi = tg._mods()[0]
    r = np.ascontiguousarray(rec, _capi.PHOTO_ROBUST_DTYPE).reshape(1)
    out72, r_px, flags = np.zeros(72, np.float32), np.zeros((8, 8)), C.c_int32(0)
    ok = rref.photo_refine_ref_measurement(C.c_void_p(r.ctypes.data), int(accepted), C.byref(o), C.c_double(k), C.c_void_p(out72.ctypes.data),
                                           C.c_void_p(r_px.ctypes.data), C.byref(flags))
    return ok, out72, r_px, flags.value


def test_refusal_at_iteration_zero_composes(blob, ref, rref):
    """c. the gate at the midpoint of the iteration-0 ratios refuses 4 of 8 sessions, refinement on for all 8.  The 4 unrefused are the ungated run's byte
    for byte.  For the 4 refused: the refine record's alignment equals, byte for byte, level 0 of hnet_sessions_photo_align_robust called afterwards from
    last_priors[0] with the same options (the NaN-started neighbours disturb nothing); r_px and the innovation agree with the host header on that record;
    the state agrees with filters_ref's propagation followed by hnet_ekf::iterated_update_photo_refined fed the step's own outputs and records;
    updates = 1, flags ASKED | APPLIED, the sequence numbers advance by iters, the statistics follow the records"""
    _capi = tg._mods()[0]
    (e, s, f), (ps, sts, imus), ids, ung, rec_u, ratio, load = _ungated(blob, [1] * 8, 81)
    inn_u = f.last_innovations(8)
    gate, above = _midpoint_gate(ratio)
    o = _ropts(cov_scale=4.0)
    for i in ids:
        f.set_photo_gate(int(i), gate)
        f.set_photo_refine(int(i), o)
    load()
    out, net, upd = f.step(ids, [T_FRAME] * 8, imus)
    rec_g, inn_g, rr, pri = f.last_photometric(8), f.last_innovations(8), f.last_refine(8), f.last_priors(8)
    assert f.get_state(ids).tobytes() == out.tobytes() and [s.seq(int(i)) for i in ids] == [4 + 3] * 8
    refused = [int(i) for i in np.flatnonzero(above)]
    after, lv = s.photo_align_robust(refused, pri[0][refused], levels=2, want_levels=True, max_iterations=3)
    worst_r, worst_i = 0.0, 0.0
    for i in range(8):
        if not above[i]:
            assert upd[i] == 3 and out[i].tobytes() == ung[0][i].tobytes() and rec_g[i].tobytes() == rec_u[i].tobytes()
            assert inn_g[:, i].tobytes() == inn_u[:, i].tobytes() and rr[i].tobytes() == np.zeros(1, _capi.PHOTO_REFINE_DTYPE).tobytes()
            continue
        k = refused.index(i)
        assert list(rec_g["flags"][i]) == [0, 0, pg.PH_REJECTED, 0, 0] and list(inn_g["flag"][:, i]) == [SKIPPED] * 3
        assert rr["flags"][i] == ASKED | APPLIED and rr["pad"][i] == 0 and upd[i] == 1, (i, rr["flags"][i], upd[i])
        assert rr["rec"][i].tobytes() == after[k].tobytes(), i                 # the pinned identity
        assert rr["rec"][i]["px"]["accepted"] > 0 and not rr["rec"][i]["px"]["flags"] & (U.SINGULAR | U.DEGENERATE | U.FEW_PIXELS)
        accepted = int(lv[k]["px"]["accepted"].sum())
        ok, m72, r_px, fl = _host_measure(rref, rr["rec"][i], accepted, o, ps[i].k_net_cov)
        assert ok == 1 and fl == 0
        rel = float(np.abs(rr["r_px"][i] - r_px).max() / np.abs(r_px).max())
        worst_r = max(worst_r, rel)
        # the host loop: propagation, then iterated_update_photo_refined with this step's outputs, its records and the device's alignment as the aligner
        st = np.array(sts[i], dtype=_capi.FILTER_STATE_DTYPE).reshape(1).copy()
        r = np.ascontiguousarray(imus[i])
        assert ref.ref_propagate_with_imu(C.c_void_p(st.ctypes.data), C.byref(ps[i]), C.c_double(T_FRAME), C.c_void_p(r.ctypes.data), len(r)) >= 0
        hinn = np.zeros(1, _capi.INNOVATION_DTYPE)
        assert rref.photo_refine_ref_innovation(C.c_void_p(st.ctypes.data), C.byref(ps[i]), C.c_void_p(m72.ctypes.data), C.c_void_p(hinn.ctypes.data)) == 1
        rel_i = max(ti._rel(rr["innov"][fld][i], hinn[fld][0]) for fld in ("r", "s_diag", "nis"))
        worst_i = max(worst_i, rel_i)
        assert rr["innov"]["flag"][i] == USED and rr["innov"]["iteration"][i] == 3 and np.isfinite(rr["innov"]["nis"][i])
        nn = np.ascontiguousarray(net[:, i, :], dtype=np.float32)
        script = np.ascontiguousarray(pg._unflag(rec_g)[i, 1:])
        arec = np.ascontiguousarray(rr["rec"][i]).reshape(1)
        hin, hrec, hout = np.zeros(3, _capi.INNOVATION_DTYPE), np.zeros(4, _capi.PHOTO_RESIDUAL_DTYPE), np.zeros(1, _capi.PHOTO_REFINE_DTYPE)
        x0 = np.zeros(8, np.float32)
        u = rref.photo_refine_ref_iterated(C.c_void_p(st.ctypes.data), C.byref(ps[i]), 3, C.c_void_p(nn.ctypes.data), 1, C.c_double(0.0), C.c_void_p(script.ctypes.data),
                                           C.c_double(gate), 0, C.byref(o), C.c_void_p(arec.ctypes.data), accepted, C.c_void_p(hin.ctypes.data),
                                           C.c_void_p(hrec.ctypes.data), C.c_void_p(hout.ctypes.data), None, None, C.c_void_p(x0.ctypes.data))
        assert u == 1 and hout["flags"][0] == rr["flags"][i] and list(hrec["flags"]) == list(rec_g["flags"][i, 1:])
        assert np.abs(x0 - pri[0][i]).max() <= 1e-6 * max(1.0, np.abs(x0).max())  # (the host's fp32 prior comes from its own propagation)
        tg._close(out[i], st[0])
        print(f"session {i}: r_px rel {rel:.2e}, innovation rel {rel_i:.2e}, NIS {rr['innov']['nis'][i]:.3f}, accepted {accepted}, mse {rr['rec'][i]['px']['mse']:.3f}")
    print(f"worst r_px relative difference {worst_r:.2e}, worst innovation relative difference {worst_i:.2e}")
    assert worst_r <= 10 * MEASURED_RPX and worst_i <= 10 * MEASURED_INNOV
    _check_stats(f, ids, [rr])
    pg._check_stats(f, ids, [(rec_u, ung[2], inn_u), (rec_g, upd, inn_g)])
    for x in (f, s, e):
        x.close()


# ---- d: it helps --------------------------------------------------------------------------------------------------------------------------------------

def test_refined_offsets_reach_the_truth(blob):
    """d. states with zero offsets (the prior is 0 px), the smooth pairs of max_offset 2 for seeds 1, 2, 5, 11 (two sessions each, with different mask
    sequence numbers), the gate chosen as in c: every refused and refined session's offsets lie within 0.05 px of the truth (DESIGN 7k's gate for this pair
    family; the host reference ends 0.013 - 0.019 px off at these options) and its NIS is finite; at least 2 sessions must have been refused and applied"""
    seeds = [1, 2, 5, 11, 1, 2, 5, 11]
    (e, s, f), (ps, sts, imus), ids, ung, rec_u, ratio, load = _ungated(blob, seeds, 83, zero_offsets=True, seqs=[4 + 10 * i for i in range(8)])
    gate, above = _midpoint_gate(ratio)
    for i in ids:
        f.set_photo_gate(int(i), gate)
        f.set_photo_refine(int(i), _ropts())
    load()
    out, net, upd = f.step(ids, [T_FRAME] * 8, imus)
    rr, pri = f.last_refine(8), f.last_priors(8)
    assert not pri[0].any()
    done = 0
    for i in range(8):
        if not rr["flags"][i] & ASKED:
            assert not above[i]
            continue
        assert above[i] and rr["flags"][i] == ASKED | APPLIED and upd[i] == 1, (i, rr["flags"][i])
        err = float(np.abs(rr["rec"][i]["px"]["offsets_px"].astype(np.float64) - U.smooth_pair(seeds[i], 2.0)[2]).max())
        print(f"session {i} (seed {seeds[i]}): {err:.4f} px off, NIS {rr['innov']['nis'][i]:.3f}, sqrt diag R {np.sqrt(np.diag(rr['r_px'][i])).round(4)}")
        assert err < 0.05 and np.isfinite(rr["innov"]["nis"][i])
        done += 1
    assert done >= 2, rr["flags"]
    for x in (f, s, e):
        x.close()


# ---- e: unusable and gated fallbacks in one call --------------------------------------------------------------------------------------------------------

def test_unusable_gated_and_off_in_one_call(blob):
    """e. all 8 sessions refused at iteration 0 (a gate of 1e-6).  Session 0's current frame is constant (the alignment stops SINGULAR: unusable), 1 has a NIS
    gate of 1e-30, 2 a max_mse of 1e-30, 3 has refinement off: each ends, byte for byte, in the state a step with the reference gate closed leaves, with
    updates 0.  Sessions 4 - 7 are refined and applied, and keep their bytes when 0 - 3 are absent from the call"""
    _capi = tg._mods()[0]
    const = np.full((224, 320), 93, np.uint8)
    e, s, f = pg._fleet(blob, 3, True)
    ec, sc, fc = pg._track(*tg._setup(blob, 8, 3, frames=6))                  # 8 images with the pair: the reference gate stays closed
    for ss in (s, sc):
        _push_pairs(ss, [1] * 8, {0: const})
    ps, sts, imus = _inputs(85)
    ids = np.arange(8, dtype=np.int32)
    for i in range(8):
        f.set_photo_gate(i, 1e-6)
        if i != 3:
            f.set_photo_refine(i, _ropts(max_mse=1e-30 if i == 2 else 0.0))
    f.set_nis_gate(1, 1e-30)
    ti._load(f, s, ps, sts, seq=4)
    ti._load(fc, sc, ps, sts, seq=4)
    out, net, upd = f.step(ids, [T_FRAME] * 8, imus)
    rr, rec = f.last_refine(8), f.last_photometric(8)
    closed = fc.step(ids, [T_FRAME] * 8, imus)
    assert list(closed[2]) == [0] * 8 and all(list(rec["flags"][i]) == [0, 0, pg.PH_REJECTED, 0, 0] for i in range(8))
    print("flags", list(rr["flags"]), "updates", list(upd), "level-0 flags", list(rr["rec"]["px"]["flags"]))
    assert rr["flags"][0] == ASKED | STOPPED and rr["rec"][0]["px"]["flags"] & U.SINGULAR and not rr["r_px"][0].any() and rr["innov"]["flag"][0] == NONE
    assert rr["flags"][1] == ASKED | NIS_REJECTED and rr["innov"]["flag"][1] == REJECTED and rr["innov"]["nis"][1] > 1e-30
    assert rr["flags"][2] == ASKED | MSE_ABOVE_MAX and not rr["r_px"][2].any()
    assert rr[3].tobytes() == np.zeros(1, _capi.PHOTO_REFINE_DTYPE).tobytes()
    for i in range(4):
        assert upd[i] == 0 and out[i].tobytes() == closed[0][i].tobytes(), i
    for i in range(4, 8):
        assert rr["flags"][i] == ASKED | APPLIED and upd[i] == 1 and out[i].tobytes() != closed[0][i].tobytes()
    assert all(rr["innov"]["iteration"][i] == 3 for i in (0, 1, 2, 4, 5, 6, 7))
    _check_stats(f, ids, [rr])
    assert f.innovation_stats(1)["rejected"] == 0                              # (the fallback's NIS rejection is the refine statistics', not the innovation records')
    # batch independence: the four applied sessions alone, in other slots
    ti._load(f, s, ps, sts, seq=4)
    sub = np.arange(4, 8, dtype=np.int32)
    out2, net2, upd2 = f.step(sub, [T_FRAME] * 4, imus[4:])
    rr2 = f.last_refine(4)
    assert out2.tobytes() == out[4:].tobytes() and rr2.tobytes() == rr[4:].tobytes() and list(upd2) == [1] * 4
    assert _capi.lib().hnet_filters_last_refine(f._f, 8, np.zeros(8, _capi.PHOTO_REFINE_DTYPE).ctypes.data) == INVALID      # a wrong n
    for x in (f, fc, s, sc, e, ec):
        x.close()


# ---- f: advance and repeat ------------------------------------------------------------------------------------------------------------------------------

def test_advance_equals_step(blob):
    """f. three hnet_filters_advance ticks on rings that wrap, every session refused at iteration 0 in every tick (a gate of 1e-6) and refined: states,
    outputs, updates, every kind of record and the refine statistics are those of hnet_filters_step calls with the windows taken from the full history.
    The first tick's pair is a smooth pair (some fallback is applied); the later frames are other textures, whatever the alignment makes of them"""
    _capi = tg._mods()[0]
    iters = 3
    ea, sa, fa = pg._fleet(blob, iters, True)
    eb, sb, fb = pg._fleet(blob, iters, True)
    ps, _, hist, t_frame = _advance_rig([(sa, fa), (sb, fb)], 29, 1e-6, 3 * 42 + 4)
    ids = np.arange(8, dtype=np.int32)                                          # (the step fleet's rings stay empty)
    for f in (fa, fb):
        for i in range(8):
            f.set_photo_refine(i, _ropts(cov_scale=2.0))
    frames = [U.smooth_pair(1, 2.0)[1], U.smooth_pair(2, 2.0)[1], U.smooth_pair(5, 2.0)[1]]
    for s in (sa, sb):
        s.push(ids, np.repeat(U.smooth_pair(1, 2.0)[0][None], 8, 0), t=[pg.T_FRAME + 0.0001] * 8)   # the previous frame of tick 0, which no call advances to
    fed, calls = [0] * 8, []
    for tick in range(3):
        t_frame = t_frame + 0.002 * np.maximum(COUNTS, 0.1) + 0.0004
        for s in (sa, sb):
            s.push(ids, np.repeat(frames[tick][None], 8, 0), t=list(t_frame))
        fa.feed_imu(ids, _chunks(hist, ps, t_frame, fed))
        a = fa.advance(ids)
        b = fb.step(ids, list(t_frame), [hist[i][:fed[i]] for i in range(8)])
        assert list(a[3]) == [_capi.ADV_STEPPED] * 8
        assert _everything(fa, sa, ids, a[:3], True) == _everything(fb, sb, ids, b, True), tick
        ra, rb = fa.last_refine(8), fb.last_refine(8)
        assert ra.tobytes() == rb.tobytes() and np.all(ra["flags"] & ASKED), tick
        assert all(int(a[2][i]) == (1 if ra["flags"][i] & APPLIED else 0) for i in range(8))
        print(f"tick {tick}: flags {list(ra['flags'])}")
        calls.append(ra)
    assert np.any(calls[0]["flags"] & APPLIED) and max(fed) > 64
    for f in (fa, fb):
        _check_stats(f, ids, calls)
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


def test_repeat_counts_once(blob):
    """f. the overflowing iterative model of pg.test_repeat_counts_once with every session refused at iteration 0 and refined: the step demotes the model once
    and repeats the attempt, the fallback with it; refine records, states and statistics are those of fresh objects whose iterative engine runs
    HNET_PREC_BF16X3 from the start, each fallback counted once"""
    from cuahn_vio_amd.homography_net import HnetEngine
    _capi, _, _, HnetFilters = tg._mods()
    iters, n = 3, 4
    ov = ic.overflow_iterative_blob()
    ps, sts, imus = ti._inputs(_capi, HnetFilters, 47, n, T_FRAME, [16])
    ids = np.arange(n, dtype=np.int32)
    res = []
    for prec in (pg.PREC_F16X2, pg.PREC_BF16X3):
        e, s, f = tg._setup(blob, n, iters, precision=pg.PREC_F16X2)
        ie = HnetEngine(ov, variant="prior1", mc_samples=8, dropout_p=0.1, mc_seed=9, max_batch=8, precision=prec)
        pg._track(e, ie, s, f)
        s.set_iterative_model(ie)
        f.enable_photometric()
        _push_pairs(s, [1, 2, 5, 11])
        for i in ids:
            f.set_photo_gate(int(i), 1e-6)
            f.set_photo_refine(int(i), _ropts())
        ti._load(f, s, ps, sts)
        out, net, upd = f.step(ids, [T_FRAME] * n, imus)
        rr = f.last_refine(n)
        assert ie.precision() == pg.PREC_BF16X3 and e.precision() == pg.PREC_F16X2      # (demoted once, the iterative context only)
        assert [s.seq(int(i)) for i in ids] == [iters] * n and np.all(np.isfinite(net)) and np.all(rr["flags"] & ASKED)
        stats = [f.refine_stats(int(i)) for i in ids]
        assert all(st["asked"] == 1 for st in stats)
        _check_stats(f, ids, [rr])
        res.append((out, net, upd, rr, stats))
        for o in (f, s, ie, e):
            o.close()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(res[0][:4], res[1][:4])) and res[0][4] == res[1][4]
    assert np.any(res[0][3]["flags"] & APPLIED)


# ---- g: errors -------------------------------------------------------------------------------------------------------------------------------------------

def test_errors(blob):
    """g. every HNET_ERR_INVALID_ARG of set_photo_refine, the accessors and a step whose refining sessions differ in align / levels: nothing changed - the
    step that follows is the one of a fleet that never heard of refinement"""
    _capi, _, _, HnetFilters = tg._mods()
    ea, sa, fa = pg._track(*tg._setup(blob, 8, 1))
    eb, sb, fb = pg._track(*tg._setup(blob, 8, 1))
    L = _capi.lib()
    st = _capi.RefineStats()
    good = _ropts()
    buf = np.zeros(8, _capi.PHOTO_REFINE_DTYPE)
    assert L.hnet_filters_set_photo_refine(fa._f, 0, C.byref(good)) == INVALID                  # before hnet_filters_enable_photometric
    for f in (fa, fb):
        f.enable_innovations()
        f.enable_photometric()
    assert L.hnet_filters_refine_stats(fa._f, 0, C.byref(st)) == INVALID and L.hnet_filters_reset_refine_stats(fa._f, 0) == INVALID      # never turned on
    assert L.hnet_filters_last_refine(fa._f, 8, buf.ctypes.data) == INVALID
    for bad_id in (-1, 8):
        assert L.hnet_filters_set_photo_refine(fa._f, bad_id, C.byref(good)) == INVALID
        assert L.hnet_filters_set_photo_refine(fa._f, bad_id, None) == INVALID
    assert L.hnet_filters_set_photo_refine(fa._f, 0, C.byref(_capi.photo_refine_opts())) == INVALID      # the defaults: cov_scale = 0
    for kw in (dict(levels=0), dict(levels=5), dict(cov_scale=-1.0), dict(cov_scale=float("nan")), dict(cov_scale=float("inf")), dict(sigma_floor_px=-0.1),
               dict(sigma_floor_px=float("nan")), dict(max_mse=-1.0), dict(max_mse=float("inf")), dict(huber_k=-1.0), dict(max_iterations=33), dict(brightness=2),
               dict(brightness=0, gain0=1.1)):
        assert L.hnet_filters_set_photo_refine(fa._f, 0, C.byref(_ropts(**kw))) == INVALID, kw
    fa.set_photo_refine(5, None)                                                # off before it was ever on: accepted, and nothing is allocated
    assert L.hnet_filters_refine_stats(fa._f, 5, C.byref(st)) == INVALID
    # sessions 2 and 6 on with different levels, 4 with another huber_k: a step listing two that differ is refused; the states, times and sequence numbers stay
    ps, sts, imus = ti._inputs(_capi, HnetFilters, 61, 8, pg.T_FRAME, COUNTS)
    ids = np.arange(8, dtype=np.int32)
    for f, s in ((fa, sa), (fb, sb)):
        ti._load(f, s, ps, sts, seq=7)
        for i in ids:
            f.set_photo_gate(int(i), 1e30)
    fa.set_photo_refine(2, _ropts(levels=2))
    fa.set_photo_refine(6, _ropts(levels=3))
    assert L.hnet_filters_refine_stats(fa._f, 8, C.byref(st)) == INVALID and L.hnet_filters_reset_refine_stats(fa._f, -1) == INVALID
    before = fa.get_state(ids).tobytes()
    with pytest.raises(_capi.HnetError) as err:
        fa.step(ids, [pg.T_FRAME] * 8, imus)
    assert err.value.status == INVALID and fa.get_state(ids).tobytes() == before and [sa.seq(int(i)) for i in ids] == [7] * 8
    fa.set_photo_refine(6, _ropts(levels=2, huber_k=5.0))
    with pytest.raises(_capi.HnetError) as err:
        fa.step(ids, [pg.T_FRAME] * 8, imus)
    assert err.value.status == INVALID and fa.get_state(ids).tobytes() == before
    sub = np.array([0, 1, 2, 3], np.int32)                                      # a call that lists only one of the two is served
    fa.step(sub, [pg.T_FRAME] * 4, imus[:4])
    assert L.hnet_filters_last_refine(fa._f, 8, buf.ctypes.data) == INVALID and not fa.last_refine(4)["flags"].any()
    fa.set_photo_refine(2, None)
    fa.set_photo_refine(6, None)
    for f, s in ((fa, sa), (fb, sb)):
        ti._load(f, s, ps, sts, seq=7)
    a, b = fa.step(ids, [pg.T_FRAME] * 8, imus), fb.step(ids, [pg.T_FRAME] * 8, imus)
    assert _everything(fa, sa, ids, a, True) == _everything(fb, sb, ids, b, True) and list(a[2]) == [1] * 8
    assert L.hnet_filters_last_refine(fa._f, 8, buf.ctypes.data) == INVALID      # the last call ran without a refining session
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


def test_mismatch_is_refused_by_advance(blob):
    """g. hnet_filters_advance with two stepping sessions whose alignment options differ: HNET_ERR_INVALID_ARG, states, times and sequence numbers as they
    were; with the options made equal the same frame is then served"""
    _capi = tg._mods()[0]
    e, s, f = pg._fleet(blob, 1, False)
    ps, _, hist, t_frame = _advance_rig([(s, f)], 31, 1e30, 50)
    ids = np.arange(8, dtype=np.int32)
    f.set_photo_refine(2, _ropts(levels=2))
    f.set_photo_refine(6, _ropts(levels=3))
    t_frame = t_frame + 0.002 * np.maximum(COUNTS, 0.1) + 0.0004
    s.push(ids, np.repeat(tg._frames(np.random.default_rng(7), 1), 8, 0), t=list(t_frame))
    f.feed_imu(ids, _chunks(hist, ps, t_frame, [0] * 8))
    before, seqs = f.get_state(ids).tobytes(), [s.seq(int(i)) for i in ids]
    with pytest.raises(_capi.HnetError) as err:
        f.advance(ids)
    assert err.value.status == INVALID and f.get_state(ids).tobytes() == before and [s.seq(int(i)) for i in ids] == seqs
    f.set_photo_refine(6, _ropts(levels=2))
    out, net, upd, status = f.advance(ids)
    assert list(status) == [_capi.ADV_STEPPED] * 8 and list(upd) == [1] * 8 and not f.last_refine(8)["flags"].any()
    for o in (f, s, e):
        o.close()
