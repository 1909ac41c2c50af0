"""hnet_filters with recovery inside the in-step keyframe track (include/hnet.h hnet_filters_set_keyframe_recover;
csrc/kernels_filters_keyframe.hip).  A fleet that measures and never heard of it, one that set and cleared it and one where it is on
and nobody is lost must agree byte for byte; per frame of 7u's four rows the in-step track must be hnet_sessions_keyframe_track_recover's with the
filter's own step on a sessions object that is not run under the filter - records, keyframe, map - the measurement the host header's on the device's
records, and the flags those of the host rows; a mixed call out of order; a repeated attempt; advance against step; the NIS gate on the jumped frame;
every refusal.  4 cameras, max_batch 8, map capacity 3, 1 iteration unless stated."""
import ctypes as C

import numpy as np
import pytest

import filters_keyframe_recover_util as FR
import filters_keyframe_util as FK
import keyframe_recover_util as KR
import photo_search_oriented_util as O
import test_gpu_filters as tg
import test_gpu_filters_innov as ti
import test_gpu_filters_keyframe as gk
import test_gpu_filters_photo_gate as pg
import test_gpu_filters_photo_refine as pr
import test_sessions_iterative_cpu as ic
from test_gpu_filters_photo_gate import _close_in_order  # noqa: F401  (autouse: closes what pg._track holds, the last one first)

pytestmark = pytest.mark.gpu

INVALID = 1
T0 = gk.T0
EMPTY = gk.EMPTY
CAPACITY = 3
# z_px, r_px and the innovation of every applied frame of the rows, device against the host header on the device's records, relative as ti._rel: all 0
# (the two sides share the code and the 8x8 inverse is pinned by DESIGN 7l).  Gates: 10 x, which is equality
MEASURED_Z = MEASURED_RPX = MEASURED_INNOV = 0.0


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ti._build(tmp_path_factory.mktemp("filters_ref_kfr"), "filters_ref")


@pytest.fixture(scope="module")
def klib(tmp_path_factory):
    return FK.build_ref(tmp_path_factory.mktemp("filters_keyframe_ref_kfr"))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return FR.build_ref(tmp_path_factory.mktemp("filters_keyframe_recover_ref_gpu"))


def _zero_reloc():
    z = np.zeros(1, O.ORELOC)
    z["target"] = -2
    return z[0]


def _rig(blob, iters, n, capacity, k_net_cov=1e12):
    return gk._rig(blob, iters, n, map_capacity=capacity, k_net_cov=k_net_cov)


def _twin_sessions(blob, n, capacity):
    """a sessions object that is not run under the filter: the tracks are made by hand on it"""
    e2, s2, f2 = pg._track(*tg._setup(blob, n, 1))
    s2.enable_keyframes()
    if capacity:
        s2.enable_keyframe_map(capacity)
    return e2, s2, f2


def _store(s, ids, capacity):
    """keyframe images, map tables and the valid map images of the sessions ids"""
    out = []
    for i in ids:
        item = [s.keyframe(int(i)).tobytes()]
        if capacity:
            en, ms = s.keyframe_map_info(int(i))
            item += [en.tobytes(), ms.tobytes()] + [s.map_keyframe(int(i), slot).tobytes() for slot in range(capacity) if en["valid"][slot]]
        out.append(item)
    return out


def _posterior(ref, klib, st, p, t, net72):
    """the host's state after propagation without an interval and the network's one update with update_offset = 1 (the reference gate is open)"""
    _capi = tg._mods()[0]
    s = np.array(st, dtype=_capi.FILTER_STATE_DTYPE).reshape(1).copy()
    assert ref.ref_propagate_with_imu(C.c_void_p(s.ctypes.data), C.byref(p), C.c_double(t), C.c_void_p(EMPTY.ctypes.data), 0) >= 0
    ok, post = FK.ref_update(klib, s, p, net72, 1, 0)
    assert ok == 1
    return post


# ---- 1: the four rows x four seeds in one call of four slots ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", KR.ROWS)
def test_rows_on_the_device(blob, ref, klib, lib, name):
    """one session per seed.  Per frame: m.track and reloc equal hnet_sessions_keyframe_track_recover made by hand with the record's step_px on a second
    sessions object, and so do the keyframe, the map's tables and images; z_px, r_px and the innovation equal the host header's on the device's records
    (relative difference 0); flags and prev_ok behave as on the host rows (tests/test_filters_keyframe_recover_cpu.py); the figure of the frame after the
    recovery equals the host row's to the printed digit.  A plain track that follows gives the same record on both objects."""
    _capi = tg._mods()[0]
    n, cap = 4, KR.capacity(name)
    (e, s, f), ps, rng = _rig(blob, 1, n, cap)
    e2, s2, f2 = _twin_sessions(blob, n, cap)
    ids = np.arange(n, dtype=np.int32)
    mo, ro = FR.row_measure_opts(name), KR.reloc_opts(name)
    for i in ids:
        f.set_keyframe_measure(int(i), mo)
        f.set_keyframe_recover(int(i), ro)
    rows = [KR.row(name, sd) for sd in KR.SEEDS]
    r0 = rows[0]
    prev_ok, had_key, key_prev = [0] * n, [False] * n, [np.zeros(8, np.float32) for _ in range(n)]
    worst = dict(z=0.0, r_px=0.0, innov=0.0)
    for fi in range(len(r0["frames"])):
        t = T0 + 0.1 * fi
        frames = [rows[k]["frames"][fi] for k in range(n)]
        states = [FK.row_state(FR.row_step(rows[k], fi), t - 0.05) for k in range(n)]
        keys_before = [s2.keyframe(int(i)) if had_key[k] else None for k, i in enumerate(ids)]
        out, net, upd = gk._tick(s, f, ids, frames, t, states)
        rr = f.last_keyframe_recover(n)
        assert f.last_keyframe_measure(n).tobytes() == rr["m"].tobytes()
        s2.push(ids, np.stack(frames), t=[t] * n)
        hand = s2.keyframe_track_recover(ids, step_px=rr["m"]["step_px"], track=mo.track, reloc=ro)
        assert hand["track"].tobytes() == rr["m"]["track"].tobytes(), (fi, [hex(int(x)) for x in hand["track"]["flags"]], [hex(int(x)) for x in rr["m"]["track"]["flags"]])
        assert hand["reloc"].tobytes() == rr["reloc"].tobytes(), fi
        assert _store(s, ids, cap) == _store(s2, ids, cap), fi
        print(f"{name}, frame {fi}: flags {[hex(int(x)) for x in rr['m']['flags']]}, track {[hex(int(x)) for x in rr['m']['track']['flags']]}, "
              f"reloc {[hex(int(x)) for x in rr['reloc']['rv']['flags']]}, updates {list(upd)}")
        for k, i in enumerate(ids):
            r, m = rr[k], rr[k]["m"]
            tfl, rfl, fl = int(m["track"]["flags"]), int(r["reloc"]["rv"]["flags"]), int(m["flags"])
            acc, acc2 = 0, 0
            if had_key[k]:
                op, lv = e.op_photo_align_robust(keys_before[k], frames[k], m["track"]["start_px"], levels=mo.track.levels, want_levels=True,
                                                 max_iterations=mo.track.align.base.max_iterations)
                acc = int(lv[0]["px"]["accepted"].sum())
            if rfl & _capi.RL_RETRACKED:
                op, lv = e.op_photo_align_robust(keys_before[k], frames[k], r["reloc"]["search"]["base"]["start_px"], levels=ro.levels, want_levels=True,
                                                 max_iterations=ro.align.base.max_iterations)
                acc2 = int(lv[0]["px"]["accepted"].sum())
            ok, z, r_px, m72, why = FR.ref_measure(lib, had_key[k], key_prev[k], prev_ok[k], m["track"], acc, r["reloc"], acc2, mo, ps[k].k_net_cov)
            assert fl & (FR.UNUSABLE | FR.FROM_RELOC) == why and m["pad"] == 0, (fi, k, hex(fl), hex(why))
            if ok:
                assert fl & ~FR.FROM_RELOC == FK.ASKED | FK.APPLIED and upd[k] == 2, (fi, k, hex(fl))
                post = _posterior(ref, klib, states[k], ps[k], t, net[0, k])
                inn = FR.ref_innovation(lib, post, ps[k], z, r_px)
                worst["z"] = max(worst["z"], ti._rel(m["z_px"], z))
                worst["r_px"] = max(worst["r_px"], float(np.abs(m["r_px"] - r_px).max() / np.abs(r_px).max()))
                worst["innov"] = max(worst["innov"], max(ti._rel(m["innov"][fld], inn[fld]) for fld in ("r", "s_diag", "nis")))
                assert m["innov"]["flag"] == FK.INN_USED and m["innov"]["iteration"] == 1
            else:
                assert not m["z_px"].any() and not m["r_px"].any() and m["innov"]["flag"] == FK.INN_NONE and upd[k] == 1
            # the rows' table
            lost, const, nxt = rows[k]["lost"], rows[k]["constant"], rows[k]["next"]
            if fi == 0:
                assert fl == FK.ASKED | FK.FIRST
            elif fi == lost and const is None:
                assert fl == FK.ASKED | FK.APPLIED | FR.FROM_RELOC and tfl & _capi.KF_LOST and tfl & _capi.KF_RECOVERED and rfl == _capi.RL_RETRACKED, (k, hex(fl))
                assert m["z_px"].tobytes() == r["reloc"]["rv"]["key_px"].tobytes()           # (the previous key_px is zero)
                assert float(np.abs(m["z_px"].astype(np.float64) - rows[k]["pose"]).max()) <= KR.gate(name)
            elif fi == const:
                assert fl == FK.ASKED | FK.TRACK_LOST and not tfl & _capi.KF_RECOVERED and r["reloc"]["rv"]["flags"] & _capi.RL_NO_CANDIDATE
            elif fi == lost:
                assert fl == FK.ASKED | FR.REATTACHED and tfl & _capi.KF_RECOVERED and rfl == _capi.RL_ATTACHED, (k, hex(fl))
            else:
                assert fl == FK.ASKED | FK.APPLIED and not tfl & _capi.KF_LOST, (fi, k, hex(fl))
                assert r["reloc"].tobytes() == _zero_reloc().tobytes()
            if fi == nxt:
                err, host = FR.next_z_error(name, KR.SEEDS[k], m["z_px"]), FR.NEXT_Z[name][k]
                print(f"  seed {KR.SEEDS[k]}: z_px of the frame after the recovery {err:.4f} px off (host {host:.4f})")
                assert abs(err - host) <= 1e-4 and err <= FR.next_z_gate(name)
            # the host's bookkeeping for the next frame: key_px from the second object, prev_ok by the rule
            prev_ok[k] = 0 if (tfl & _capi.KF_LOST and not tfl & _capi.KF_RECOVERED) else 1
            had_key[k] = True
        for k in range(n):                                                      # the session's key_px after the call: the relocalise's, zero behind a re-key, else the record's
            tfl = int(rr[k]["m"]["track"]["flags"])
            key_prev[k] = (rr[k]["reloc"]["rv"]["key_px"] if tfl & _capi.KF_RECOVERED else np.zeros(8, np.float32) if tfl & _capi.KF_REKEYED
                           else rr[k]["m"]["track"]["key_px"]).copy()
        assert f.keyframe_measure_stats(0)["asked"] == fi + 1
    print(f"worst: z rel {worst['z']:.2e}, r_px rel {worst['r_px']:.2e}, innovation rel {worst['innov']:.2e}")
    assert worst["z"] <= 10 * MEASURED_Z and worst["r_px"] <= 10 * MEASURED_RPX and worst["innov"] <= 10 * MEASURED_INNOV
    st = f.keyframe_measure_stats(0)
    want_unusable = 1 if r0["constant"] is None else 3                            # FIRST; and TRACK_LOST, REATTACHED with a map
    assert st["unusable"] == want_unusable and st["applied"] == len(r0["frames"]) - want_unusable
    extra = [rows[k]["frames"][r0["next"]] for k in range(n)]
    for ss in (s, s2):
        ss.push(ids, np.stack(extra), t=[T0 + 2.0] * n)
    a, b = s.keyframe_track(ids, **gk._track_kw(mo)), s2.keyframe_track(ids, **gk._track_kw(mo))
    assert a.tobytes() == b.tobytes() and not np.any(a["flags"] & _capi.KF_GAP)
    for x in (f, f2, s, s2, e, e2):
        x.close()


# ---- 2: never heard of it --------------------------------------------------------------------------------------------------------------------------------------

def _configure(s, f, mode):
    s.enable_keyframes()
    s.enable_keyframe_map(CAPACITY)
    for i in range(8):
        f.set_keyframe_measure(i, gk._mopts())
    if mode in ("cleared", "idle"):
        for i in range(8):
            f.set_keyframe_recover(i, KR.reloc_opts("kidnapped"))
    if mode == "cleared":
        for i in range(8):
            f.set_keyframe_recover(i, None)


def _all(f, s, ids, got):
    n = len(ids)
    return gk._slots(f, s, ids, got, range(n)) + [f.last_keyframe_measure(n).tobytes()] + _store(s, ids, CAPACITY)


def _check_fleets(fleets, ids, results, tick):
    _capi = tg._mods()[0]
    (sa, fa), (sb, fb), (sc, fc) = fleets
    a, b, c = results
    assert _all(fa, sa, ids, a) == _all(fb, sb, ids, b) == _all(fc, sc, ids, c), tick
    buf = np.zeros(8, FR.RECORD)
    for f in (fa, fb):
        assert _capi.lib().hnet_filters_last_keyframe_recover(f._f, 8, buf.ctypes.data) == INVALID
    rr = fc.last_keyframe_recover(8)
    assert rr["m"].tobytes() == fa.last_keyframe_measure(8).tobytes() and all(r.tobytes() == _zero_reloc().tobytes() for r in rr["reloc"])
    assert not np.any(rr["m"]["track"]["flags"] & _capi.KF_LOST) and np.all(rr["m"]["flags"] & FK.ASKED)


@pytest.mark.parametrize("iters", [1, 3])
def test_never_heard_of_it_step(blob, iters):
    """two steps of three fleets whose 8 sessions all measure: one that never calls the new API, one that set and cleared recovery, one where it is on
    and nobody is lost - states, outputs, priors, updates, sequence numbers, innovation, photometric and measure records, keyframes and maps byte-equal;
    the third fleet's relocalise records are zero_reloc and the first two refuse hnet_filters_last_keyframe_recover"""
    _capi, _, _, HnetFilters = tg._mods()
    rigs = [pg._fleet(blob, iters, True) for _ in range(3)]
    ids = np.arange(8, dtype=np.int32)
    frames = gk._seq_frames()
    ps, sts, imus = ti._inputs(_capi, HnetFilters, 90 + iters, 8, T0, gk.COUNTS)
    for p in ps:
        p.k_net_cov *= gk.K_HEAVY
    rng = np.random.default_rng(7)
    t2 = [T0 + 0.002 * max(gk.COUNTS[i], 1) + 0.0004 for i in range(8)]
    imus2 = [tg._imu(rng, T0 + ps[i].cam_imu_dt, gk.COUNTS[i]) for i in range(8)]
    for (e, s, f), mode in zip(rigs, ("never", "cleared", "idle")):
        ti._load(f, s, ps, sts, seq=7)
        _configure(s, f, mode)
    fleets = [(s, f) for _, s, f in rigs]
    for tick, (t, im, fr) in enumerate((([T0] * 8, imus, frames[0]), (t2, imus2, frames[1]))):
        res = []
        for s, f in fleets:
            s.push(ids, np.repeat(fr[None], 8, 0), t=list(t))
            res.append(f.step(ids, t, im))
        _check_fleets(fleets, ids, res, tick)
    for e, s, f in rigs:
        for o in (f, s, e):
            o.close()


@pytest.mark.parametrize("iters", [1, 3])
def test_never_heard_of_it_advance(blob, iters):
    """the same for three hnet_filters_advance ticks on rings of 64 readings that wrap"""
    _capi = tg._mods()[0]
    rigs = [pg._fleet(blob, iters, True) for _ in range(3)]
    fleets = [(s, f) for _, s, f in rigs]
    ps, _, hist, t_frame = pr._advance_rig(fleets, 23, 1e30, 3 * 42 + 4)
    gk._heavy(ps, [f for _, f in fleets])
    for (s, f), mode in zip(fleets, ("never", "cleared", "idle")):
        _configure(s, f, mode)
    ids = np.arange(8, dtype=np.int32)
    fed = [0] * 8
    frames = gk._seq_frames()
    for tick in range(3):
        t_frame = t_frame + 0.002 * np.maximum(gk.COUNTS, 0.1) + 0.0004
        chunks = pr._chunks(hist, ps, t_frame, fed)
        res = []
        for s, f in fleets:
            s.push(ids, np.repeat(frames[tick][None], 8, 0), t=list(t_frame))
            f.feed_imu(ids, chunks)
            out = f.advance(ids)
            assert list(out[3]) == [_capi.ADV_STEPPED] * 8
            res.append(out[:3])
        _check_fleets(fleets, ids, res, tick)
    assert max(fed) > 64
    for e, s, f in rigs:
        for o in (f, s, e):
            o.close()


# ---- 3: the mixed call -------------------------------------------------------------------------------------------------------------------------------------------

def _drive(blob, one_per_call):
    """8 sessions, a map of 3 slots.  Sessions 1 and 6 walk the first five frames of the kidnapped_map row (6 ends lost and unrecovered on the constant
    frame), 2, 3 and 4 take the kidnapped row's keyframe; then ONE call, out of order: 5 FIRST, 2 tracked and applied, 3 lost and RETRACKED, 6 lost
    and re-attached, 1 lost and unrecovered on a constant frame, 4 measuring with recovery off and lost, 0 not measuring; 7 is not listed."""
    _capi = tg._mods()[0]
    (e, s, f), ps, _ = _rig(blob, 1, 8, CAPACITY)
    mo, ro = FR.row_measure_opts("kidnapped_map"), KR.reloc_opts("kidnapped_map")
    for i in range(1, 8):
        f.set_keyframe_measure(i, mo)
        if i != 4:
            f.set_keyframe_recover(i, ro)
    km, kd = KR.row("kidnapped_map", 5), KR.row("kidnapped", 5)
    const = np.full((224, 320), 93, np.uint8)

    def call(ids, frames, steps, t):
        groups = [np.array([i], np.int32) for i in ids] if one_per_call else [np.asarray(ids, np.int32)]
        got = {}
        for g in groups:
            sel = [list(ids).index(int(i)) for i in g]
            out, net, upd = gk._tick(s, f, g, [frames[j] for j in sel], t, [FK.row_state(steps[j], t - 0.05) for j in sel])
            recovering = any(int(i) not in (0, 4) for i in g)
            rr = f.last_keyframe_recover(len(g)) if recovering else None
            mm = f.last_keyframe_measure(len(g)) if any(int(i) != 0 for i in g) else np.zeros(len(g), FK.MEASURE)
            for k, i in enumerate(g):
                got[int(i)] = (mm[k].tobytes(), rr[k]["reloc"].tobytes() if rr is not None else _zero_reloc().tobytes(), out[k].tobytes(), int(upd[k]))
        return got

    for fi in range(5):
        call([1, 6], [km["frames"][fi]] * 2, [FR.row_step(km, fi)] * 2, T0 + 0.1 * fi)
    call([2, 3, 4], [kd["frames"][0]] * 3, [np.zeros(8, np.float32)] * 3, T0 + 0.5)
    before7 = (f.get_state(np.array([7], np.int32)).tobytes(), s.seq(7))
    order = [5, 2, 3, 6, 1, 4, 0]
    cur = {5: kd["frames"][0], 2: kd["frames"][0], 3: kd["frames"][1], 6: km["frames"][5], 1: const, 4: kd["frames"][1], 0: kd["frames"][0]}
    got = call(order, [cur[i] for i in order], [np.zeros(8, np.float32)] * 7, T0 + 0.6)
    assert (f.get_state(np.array([7], np.int32)).tobytes(), s.seq(7)) == before7
    store = _store(s, range(1, 7), CAPACITY)
    flags = {i: (int(np.frombuffer(got[i][0], FK.MEASURE)["flags"][0]), int(np.frombuffer(got[i][0], FK.MEASURE)["track"]["flags"][0])) for i in order}
    for x in (f, s, e):
        x.close()
    return got, store, flags


def test_mixed_call(blob):
    """each session of the mixed call gets what it gets alone (a twin fleet steps the sessions one per call): records, relocalise records, states, updates,
    keyframes and maps byte-equal; the session that is not listed keeps everything"""
    _capi = tg._mods()[0]
    got, store, flags = _drive(blob, False)
    print({i: (hex(a), hex(b)) for i, (a, b) in flags.items()})
    assert flags[5][0] == FK.ASKED | FK.FIRST
    assert flags[2][0] == FK.ASKED | FK.APPLIED and not flags[2][1] & _capi.KF_LOST
    assert flags[3][0] == FK.ASKED | FK.APPLIED | FR.FROM_RELOC and flags[3][1] & _capi.KF_RECOVERED
    assert flags[6][0] == FK.ASKED | FR.REATTACHED and flags[6][1] & _capi.KF_RECOVERED
    assert flags[1][0] == FK.ASKED | FK.TRACK_LOST and flags[1][1] & _capi.KF_LOST and not flags[1][1] & _capi.KF_RECOVERED
    assert flags[4][0] == FK.ASKED | FK.TRACK_LOST and flags[4][1] & _capi.KF_REKEYED and not flags[4][1] & _capi.KF_RECOVERED
    assert got[4][1] == _zero_reloc().tobytes() and got[1][1] != _zero_reloc().tobytes()
    assert flags[0] == (0, 0) and got[0][0] == np.zeros(1, FK.MEASURE).tobytes()
    got1, store1, flags1 = _drive(blob, True)
    assert flags == flags1 and got == got1 and store == store1


# ---- 4: the rest ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_repeat_counts_once(blob):
    """a REPEATED attempt on the call in which sessions are lost.  4 recovering sessions, a map of 3 slots, 3 iterations.  The keyframes and the maps are
    built first, while the sessions have no iterative model: session 0 takes the kidnapped row's keyframe, 1 and 2 walk the kidnapped_map row (1 to its
    constant frame, 2 to the frame before it), 3 takes a keyframe.  Then the overflowing iterative model of
    test_gpu_filters_keyframe.test_repeat_counts_once is attached, and the NEXT call - in which 0 is kidnapped (RETRACKED), 1 sees the far frame
    (ATTACHED to a map keyframe), 2 a constant frame (lost, unrecovered: T1's re-key, the second commit and the second map store) and 3 tracks and
    re-keys by max_age = 1 (the first commit and the first map store) -
    demotes the model once and repeats the attempt: the working copies of the state table and of the map, the pick, the attach flags, copy2 and store2
    are all formed twice and committed once.  Against fresh objects whose iterative engine runs HNET_PREC_BF16X3 from the start, i.e. a single attempt:
    one map serial per stored keyframe (sessions 2 and 3 store one each), one attach (session 1's key image is the map image of its target, its map state
    points at it), and records, states, keyframes, map tables, map images, statistics and the call that follows byte for byte"""
    from cuahn_vio_amd.homography_net import HnetEngine
    _capi, _, _, HnetFilters = tg._mods()
    iters, n = 3, 4
    ov = ic.overflow_iterative_blob()
    kd, km = KR.row("kidnapped", 5), KR.row("kidnapped_map", 5)
    const = np.full((224, 320), 93, np.uint8)
    ids = np.arange(n, dtype=np.int32)
    rng0 = np.random.default_rng(47)
    ps = [tg._params(HnetFilters, rng0, i) for i in range(n)]
    for p in ps:
        p.k_net_cov = 1e12
    mo, ro = FR.row_measure_opts("kidnapped_map"), KR.reloc_opts("kidnapped_map")
    zero = np.zeros(8, np.float32)
    res = []
    for prec in (pg.PREC_F16X2, pg.PREC_BF16X3):
        e, s, f = tg._setup(blob, n, iters, precision=pg.PREC_F16X2)
        ie = HnetEngine(ov, variant="prior1", mc_samples=8, dropout_p=0.1, mc_seed=9, max_batch=8, precision=prec)
        pg._track(e, ie, s, f)
        s.enable_keyframes()
        s.enable_keyframe_map(CAPACITY)
        for i in ids:
            f.set_params(int(i), ps[i])
            f.set_keyframe_measure(int(i), mo)
            f.set_keyframe_recover(int(i), ro)

        def call(sub, frames, steps, t):
            sub = np.asarray(sub, np.int32)
            out, net, upd = gk._tick(s, f, sub, frames, t, [FK.row_state(st, t - 0.05) for st in steps])
            return out, net, upd, f.last_keyframe_recover(len(sub))

        # the keyframes and the maps, on the main model alone
        call([0, 3], [kd["frames"][0]] * 2, [zero] * 2, T0)
        for fi in range(5):
            sub = [1, 2] if fi < 4 else [1]
            call(sub, [km["frames"][fi]] * len(sub), [FR.row_step(km, fi)] * len(sub), T0 + 0.1 * (fi + 1))
        before = _store(s, ids, CAPACITY)
        serial0 = [int(s.keyframe_map_info(int(i))[1]["serial"][0]) for i in ids]
        s.set_iterative_model(ie)
        assert ie.precision() == prec
        # the call under test: its first attempt overflows in the iterative model and is repeated
        out, net, upd, rr = call(ids, [kd["frames"][1], km["frames"][5], const, kd["frames"][0]], [zero] * n, T0 + 1.0)
        assert ie.precision() == pg.PREC_BF16X3 and e.precision() == pg.PREC_F16X2          # (demoted once, by this call, the iterative context only)
        assert np.all(np.isfinite(net))
        fl, tf, rf = ([int(x) for x in rr["m"]["flags"]], [int(x) for x in rr["m"]["track"]["flags"]], [int(x) for x in rr["reloc"]["rv"]["flags"]])
        print([hex(x) for x in fl], [hex(x) for x in tf], [hex(x) for x in rf], list(upd))
        assert fl[0] == FK.ASKED | FK.APPLIED | FR.FROM_RELOC and rf[0] == _capi.RL_RETRACKED and tf[0] & _capi.KF_RECOVERED
        assert fl[1] == FK.ASKED | FR.REATTACHED and rf[1] == _capi.RL_ATTACHED and tf[1] & _capi.KF_RECOVERED
        assert fl[2] == FK.ASKED | FK.TRACK_LOST and tf[2] & _capi.KF_REKEYED and not tf[2] & _capi.KF_RECOVERED and rf[2] & _capi.RL_NO_CANDIDATE
        assert fl[3] == FK.ASKED | FK.APPLIED and not tf[3] & _capi.KF_LOST and rr["reloc"][3].tobytes() == _zero_reloc().tobytes()
        serial1 = [int(s.keyframe_map_info(int(i))[1]["serial"][0]) for i in ids]
        assert [b - a for a, b in zip(serial0, serial1)] == [0, 0, 1, 1], (serial0, serial1)   # one map serial per stored keyframe, not two (3: max_age = 1)
        after = _store(s, ids, CAPACITY)
        assert after[0] == before[0]                                                        # RETRACKED: keyframe and map as they were
        target = int(rr["reloc"]["target"][1])
        en1, ms1 = s.keyframe_map_info(1)
        assert target >= 0 and en1["valid"][target] and int(ms1["cur_slot"][0]) == target                # one attach: the map points at the target ...
        assert s.keyframe(1).tobytes() == s.map_keyframe(1, target).tobytes() != before[1][0]            # ... and the key image is its image
        assert after[1][1] == before[1][1]                                                               # (an attach stores nothing: the entries stay)
        assert s.keyframe(2).tobytes() == const.tobytes()                                                # T1's re-key, committed once
        # the call that follows starts from what a single attempt leaves
        out2, net2, upd2, rr2 = call(ids, [kd["frames"][2], km["frames"][6], km["frames"][0], kd["frames"][0]], [FR.row_step(kd, 2), FR.row_step(km, 6), zero, zero],
                                     T0 + 1.1)
        assert rr2["m"]["flags"][0] == FK.ASKED | FK.APPLIED and rr2["m"]["flags"][1] == FK.ASKED | FK.APPLIED
        stats = [f.keyframe_measure_stats(int(i)) for i in ids]
        res.append((out.tobytes(), net.tobytes(), upd.tobytes(), rr.tobytes(), after, out2.tobytes(), upd2.tobytes(), rr2.tobytes(), _store(s, ids, CAPACITY), stats))
        for o in (f, s, ie, e):
            o.close()
    assert res[0] == res[1]


def test_advance_equals_step(blob):
    """three hnet_filters_advance ticks on rings that wrap, every session measuring and recovering, sessions 1 and 5 kidnapped on the second tick and a
    constant frame for session 2 on the third: states, outputs, updates, every kind of record, the recover records and statistics, keyframes and maps are
    those of hnet_filters_step calls with the windows taken from the full history"""
    _capi = tg._mods()[0]
    iters = 3
    ea, sa, fa = pg._fleet(blob, iters, True)
    eb, sb, fb = pg._fleet(blob, iters, True)
    ps, _, hist, t_frame = pr._advance_rig([(sa, fa), (sb, fb)], 29, 1e30, 3 * 42 + 4)
    gk._heavy(ps, (fa, fb))
    ids = np.arange(8, dtype=np.int32)
    mo, ro = FR.row_measure_opts("kidnapped"), KR.reloc_opts("kidnapped")
    for s, f in ((sa, fa), (sb, fb)):
        s.enable_keyframes()
        s.enable_keyframe_map(2)
        for i in range(8):
            f.set_keyframe_measure(i, mo)
            f.set_keyframe_recover(i, ro)
    kd = KR.row("kidnapped", 5)
    const = np.full((224, 320), 93, np.uint8)
    ticks = [[kd["frames"][0]] * 8, [kd["frames"][1] if i in (1, 5) else kd["frames"][0] for i in range(8)],
             [const if i == 2 else kd["frames"][2] if i in (1, 5) else kd["frames"][0] for i in range(8)]]
    fed, seen = [0] * 8, 0
    for tick in range(3):
        t_frame = t_frame + 0.002 * np.maximum(gk.COUNTS, 0.1) + 0.0004
        for s in (sa, sb):
            s.push(ids, np.stack(ticks[tick]), t=list(t_frame))
        fa.feed_imu(ids, pr._chunks(hist, ps, t_frame, fed))
        a = fa.advance(ids)
        b = fb.step(ids, list(t_frame), [hist[i][:fed[i]] for i in range(8)])
        assert list(a[3]) == [_capi.ADV_STEPPED] * 8
        assert pg._everything(fa, sa, ids, a[:3], True) == pg._everything(fb, sb, ids, b, True), tick
        ra, rb = fa.last_keyframe_recover(8), fb.last_keyframe_recover(8)
        assert ra.tobytes() == rb.tobytes() and np.all(ra["m"]["flags"] & FK.ASKED), tick
        print(f"tick {tick}: flags {[hex(int(x)) for x in ra['m']['flags']]}, track {[hex(int(x)) for x in ra['m']['track']['flags']]}")
        seen |= int(np.bitwise_or.reduce(ra["m"]["track"]["flags"]))
        assert _store(sa, ids, 2) == _store(sb, ids, 2)
        assert [fa.keyframe_measure_stats(i) for i in range(8)] == [fb.keyframe_measure_stats(i) for i in range(8)]
    assert seen & _capi.KF_RECOVERED and seen & _capi.KF_REKEYED and max(fed) > 64
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


def test_nis_gate_on_the_jumped_frame(blob):
    """frame 1 of the kidnapped row on two sessions: without a NIS gate the recovered measurement is applied, with max_nis = 20 it is NIS_REJECTED (the
    camera jumped) and only the network's update counts, as for a session that measures nothing under the same gate; prev_ok stays 1 either way: frame 2 is applied on both"""
    _capi = tg._mods()[0]
    kd = KR.row("kidnapped", 5)
    (e, s, f), ps, _ = _rig(blob, 1, 4, 0)
    ids = np.arange(3, dtype=np.int32)
    mo, ro = FR.row_measure_opts("kidnapped"), KR.reloc_opts("kidnapped")
    for i in (0, 1):
        f.set_keyframe_measure(i, mo)
        f.set_keyframe_recover(i, ro)
    f.set_nis_gate(1, 20.0)
    f.set_nis_gate(2, 20.0)
    for i in range(3):
        f.set_params(i, ps[0])
    for fi in range(3):
        t = T0 + 0.1 * fi
        out, net, upd = gk._tick(s, f, ids, [kd["frames"][fi]] * 3, t, [FK.row_state(FR.row_step(kd, fi), t - 0.05)] * 3)
        rr = f.last_keyframe_recover(3)
        print(fi, [hex(int(x)) for x in rr["m"]["flags"]], np.round(rr["m"]["innov"]["nis"], 1).tolist(), list(upd))
        if fi == 1:
            assert rr["m"]["flags"][0] == FK.ASKED | FK.APPLIED | FR.FROM_RELOC
            assert rr["m"]["flags"][1] == FK.ASKED | FK.NIS_REJECTED | FR.FROM_RELOC and rr["m"]["innov"]["flag"][1] == FK.INN_REJECTED and rr["m"]["innov"]["nis"][1] > 20.0
            assert [int(x) for x in upd] == [2, 1, 1]
            assert rr["m"][0]["z_px"].tobytes() == rr["m"][1]["z_px"].tobytes()
        if fi == 2:
            assert rr["m"]["flags"][0] == FK.ASKED | FK.APPLIED and rr["m"]["flags"][1] == FK.ASKED | FK.APPLIED
    assert f.keyframe_measure_stats(1)["nis_rejected"] == 1
    for x in (f, s, e):
        x.close()


def test_refusals_change_nothing(blob):
    """set before measure, a bad id, bad options or table, differing reloc options or tables in one call (step and advance's shared test), and
    hnet_filters_last_keyframe_recover after a call without a recovering session: HNET_ERR_INVALID_ARG and nothing changed - the step that follows is the
    one of a fleet that measures and never heard of recovery"""
    _capi, _, _, HnetFilters = tg._mods()
    ea, sa, fa = pg._fleet(blob, 1, True)
    eb, sb, fb = pg._fleet(blob, 1, True)
    L = _capi.lib()
    good = KR.reloc_opts("kidnapped")
    tab = _capi.photo_search_yaw_table()
    buf = np.zeros(8, FR.RECORD)

    def set_rc(f, i, o, h=tab, n=None):
        return L.hnet_filters_set_keyframe_recover(f._f, i, C.byref(o) if o is not None else None, h.ctypes.data if h is not None else None, len(h) if n is None else n)

    for s, f in ((sa, fa), (sb, fb)):
        s.enable_keyframes()
    assert set_rc(fa, 0, good) == INVALID                                       # before hnet_filters_set_keyframe_measure was ever on
    for f in (fa, fb):
        for i in range(8):
            f.set_keyframe_measure(i, gk._mopts())
    fa.set_keyframe_measure(3, None)
    assert set_rc(fa, 3, good) == INVALID                                       # a session that does not measure
    for bad_id in (-1, 8):
        assert set_rc(fa, bad_id, good) == INVALID and set_rc(fa, bad_id, None, None, 0) == INVALID
    for kw in (dict(levels=0), dict(levels=5), dict(min_overlap=1.5), dict(max_mse=-1.0), dict(max_closure_px=float("nan")), dict(huber_k=-1.0),
               dict(radius_x=31), dict(search_min_overlap=8)):
        try:
            bad = _capi.keyframe_relocalise_opts(**kw)
        except TypeError:
            continue
        assert set_rc(fa, 0, bad) == INVALID, kw
    bad_tab = tab.copy()
    bad_tab["a"][0] = np.nan
    assert set_rc(fa, 0, good, bad_tab) == INVALID and set_rc(fa, 0, good, tab, 65) == INVALID and set_rc(fa, 0, good, tab, 0) == INVALID
    assert L.hnet_filters_last_keyframe_recover(fa._f, 8, buf.ctypes.data) == INVALID
    fa.set_keyframe_measure(3, gk._mopts())
    fa.set_keyframe_recover(2, good)
    other = KR.reloc_opts("turned")
    assert bytes(other) != bytes(good)
    fa.set_keyframe_recover(6, other)
    ps, sts, imus = ti._inputs(_capi, HnetFilters, 61, 8, pg.T_FRAME, gk.COUNTS)
    ids = np.arange(8, dtype=np.int32)
    for f, s in ((fa, sa), (fb, sb)):
        ti._load(f, s, ps, sts, seq=7)
    before = fa.get_state(ids).tobytes()

    def refused(sub):
        with pytest.raises(_capi.HnetError) as err:
            fa.step(sub, [pg.T_FRAME] * len(sub), [imus[int(i)] for i in sub])
        assert err.value.status == INVALID and fa.get_state(ids).tobytes() == before and [sa.seq(int(i)) for i in ids] == [7] * 8
        with pytest.raises(_capi.HnetError):
            sa.keyframe(2)                                                      # no keyframe was taken
    refused(ids)                                                                # 2 and 6 differ in the reloc options
    fa.set_keyframe_recover(6, good, hyps=tab[:5])
    refused(np.array([6, 2], np.int32))                                         # ... and in their tables
    assert L.hnet_filters_last_keyframe_recover(fa._f, 8, buf.ctypes.data) == INVALID
    fa.set_keyframe_recover(6, None)
    fa.set_keyframe_measure(2, None)                                            # turning the measurement off turns recovery off
    fa.set_keyframe_measure(2, gk._mopts())
    a, b = fa.step(ids, [pg.T_FRAME] * 8, imus), fb.step(ids, [pg.T_FRAME] * 8, imus)
    assert pg._everything(fa, sa, ids, a, True) == pg._everything(fb, sb, ids, b, True)
    assert fa.last_keyframe_measure(8).tobytes() == fb.last_keyframe_measure(8).tobytes()
    assert L.hnet_filters_last_keyframe_recover(fa._f, 8, buf.ctypes.data) == INVALID      # the last call ran without a recovering session
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


def test_mismatch_is_refused_by_advance(blob):
    """hnet_filters_advance with two stepping recovering sessions whose reloc options differ, then whose tables differ: HNET_ERR_INVALID_ARG, states,
    times, sequence numbers and what the last_* calls describe as they were, no keyframe taken; with options and tables made equal the same frame is
    then served, and the call describes itself"""
    _capi = tg._mods()[0]
    e, s, f = pg._fleet(blob, 1, True)
    ps, _, hist, t_frame = pr._advance_rig([(s, f)], 31, 1e30, 50)
    ids = np.arange(8, dtype=np.int32)
    s.enable_keyframes()
    good, other, tab = KR.reloc_opts("kidnapped"), KR.reloc_opts("turned"), _capi.photo_search_yaw_table()
    for i in (2, 6):
        f.set_keyframe_measure(i, gk._mopts())
    f.set_keyframe_recover(2, good)
    f.set_keyframe_recover(6, other)
    t_frame = t_frame + 0.002 * np.maximum(gk.COUNTS, 0.1) + 0.0004
    s.push(ids, np.repeat(gk._seq_frames()[0][None], 8, 0), t=list(t_frame))
    f.feed_imu(ids, pr._chunks(hist, ps, t_frame, [0] * 8))
    before, seqs = f.get_state(ids).tobytes(), [s.seq(int(i)) for i in ids]
    L = _capi.lib()
    buf, mbuf = np.zeros(8, FR.RECORD), np.zeros(8, FK.MEASURE)

    def refused():
        with pytest.raises(_capi.HnetError) as err:
            f.advance(ids)
        assert err.value.status == INVALID and f.get_state(ids).tobytes() == before and [s.seq(int(i)) for i in ids] == seqs
        assert L.hnet_filters_last_keyframe_recover(f._f, 8, buf.ctypes.data) == INVALID and L.hnet_filters_last_keyframe_measure(f._f, 8, mbuf.ctypes.data) == INVALID
        with pytest.raises(_capi.HnetError):
            s.keyframe(2)                                                       # no keyframe was taken
    refused()                                                                   # the reloc options differ
    f.set_keyframe_recover(6, good, hyps=tab[:5])
    refused()                                                                   # the tables differ
    f.set_keyframe_recover(6, good)
    out, net, upd, status = f.advance(ids)
    rr = f.last_keyframe_recover(8)
    assert list(status) == [_capi.ADV_STEPPED] * 8 and list(upd) == [1] * 8
    assert [int(x) for x in rr["m"]["flags"]] == [FK.ASKED | FK.FIRST if i in (2, 6) else 0 for i in range(8)]
    assert all(r.tobytes() == _zero_reloc().tobytes() for r in rr["reloc"])
    for o in (f, s, e):
        o.close()


def test_map_enabled_after_recovery(blob):
    """a keyframe map enabled AFTER recovery was turned on (its working copies come with the enable): the kidnapped_map row on such an object gives,
    frame by frame, the records, states, keyframe and map of an object that enabled the map first - the constant frame lost, the far frame re-attached"""
    km = KR.row("kidnapped_map", 5)
    mo, ro = FR.row_measure_opts("kidnapped_map"), KR.reloc_opts("kidnapped_map")
    one = np.array([0], np.int32)
    res = []
    for late in (False, True):
        e, s, f = pg._track(*tg._setup(blob, 4, 1))
        f.enable_innovations()
        s.enable_keyframes()
        if not late:
            s.enable_keyframe_map(CAPACITY)
        f.set_keyframe_measure(0, mo)
        f.set_keyframe_recover(0, ro)
        if late:
            s.enable_keyframe_map(CAPACITY)
            f.set_keyframe_recover(0, ro)                                       # (again, with the map there: accepted)
        got = []
        for fi in range(len(km["frames"])):
            t = T0 + 0.1 * fi
            out, net, upd = gk._tick(s, f, one, [km["frames"][fi]], t, [FK.row_state(FR.row_step(km, fi), t - 0.05)])
            rr = f.last_keyframe_recover(1)
            got.append((out.tobytes(), upd.tobytes(), rr.tobytes(), _store(s, one, CAPACITY)))
            if fi == km["lost"]:
                assert rr["m"]["flags"][0] == FK.ASKED | FR.REATTACHED
        res.append(got)
        for o in (f, s, e):
            o.close()
    assert res[0] == res[1]
