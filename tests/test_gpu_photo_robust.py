"""Photometric alignment with a gain / bias model and Huber weights on the device (include/hnet.h hnet_op_photo_align_robust;
csrc/kernels_photo_align.hip): one linearisation per level and the whole trace against the host reference tests/cpp/photo_robust_ref.cpp, the
accuracy rows against the truth and against hnet_op_photo_align_pyramid, the model-off identity with that call, the hostile starts, bitwise independence of
the batch, the read-only sessions call and the refusals.  Calls of n = 1 and n = 3.  Main model prior-3, N = 16, max_batch 3."""
import ctypes as C

import numpy as np
import pytest

import photo_align_pyr_util as P
import photo_align_util as U
import photo_robust_util as R

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, CAPACITY = 1, 4, 5
LEVELS, K = 4, 8
# Measured on an MI355X (printed by test_level_linearisation_matches_reference), each gated at 10 x the measurement: K = 0, device against host reference,
# worst relative difference over the 3 pairs and 4 levels (summation order only: every product of two floats is exact in a double)
MEASURED_LIN = {"cost": 1.1e-13, "grad10": 1.3e-13, "info10": 7.7e-14, "grad": 1.9e-13, "info": 5.7e-13}
OFFSETS_VS_REFERENCE_PX = 1e-4          # final offsets, device against host reference: the issue's bound (every decision is expected equal, the difference 0)


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return R.build_ref(tmp_path_factory.mktemp("photo_robust_ref_gpu"))


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=3)
    yield e
    e.close()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / np.sqrt((b ** 2).sum()))


def _trace(r):
    x = r["px"]
    return (int(x["flags"]), int(x["trials"]), int(x["accepted"]), int(x["n_valid0"]), int(x["n_valid"]), int(r["n_outliers0"]), int(r["n_outliers"]))


def _run_in_threes(eng, i1, i2, start, levels, **kw):
    """the device call on pairs [0:3] and [3:4]: n = 3 and n = 1 -> (out [4], levels_out [4, levels])"""
    a = eng.op_photo_align_robust(i1[:3], i2[:3], start[:3], levels=levels, want_levels=True, **kw)
    b = eng.op_photo_align_robust(i1[3:], i2[3:], start[3:], levels=levels, want_levels=True, **kw)
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])


def test_level_linearisation_matches_reference(eng, rref):
    """max_iterations = 0 with levels = 4 is one linearisation per level at the start: on one smooth pair, one stock pair and one spoiled pair (exposure
    step and block), k = 10, the valid and the outlier counts equal the host reference's at every level, and the cost, grad10, info10 (Frobenius) and the
    offset block differ by summation order alone: within 10 x MEASURED_LIN, never above 1e-6"""
    s1, st = U.smooth_pair(1, 2.0), U.stock_pair(2)
    b1, b2, _, bs = R.row_pairs("block-1level")
    i1, i2 = np.stack([s1[0], st[0], b1[2]]), np.stack([s1[1], st[1], b2[2]])
    start = np.stack([np.zeros(8, np.float32), st[3], bs[2]])
    out, dev = eng.op_photo_align_robust(i1, i2, start, levels=LEVELS, want_levels=True, max_iterations=0, huber_k=10.0)
    _, ref = R.ref_run(rref, i1, i2, start, LEVELS, max_iterations=0, huber_k=10.0)
    assert out.tobytes() == dev[:, 0].tobytes()
    bad = []
    for L in range(LEVELS - 1, -1, -1):
        worst = {k: 0.0 for k in MEASURED_LIN}
        for b in range(3):
            d, r = dev[b, L], ref[b, L]
            assert _trace(d) == _trace(r) and d["px"]["flags"] == 0 and d["n_outliers0"] > 0, (b, L, _trace(d), _trace(r))
            assert d["px"]["trials"] == 0 and d["px"]["offsets_px"].tobytes() == start[b].tobytes() and d["gain"] == 1.0 and d["bias"] == 0.0
            assert (d["info10"] == d["info10"].T).all() and d["info10"][:8, :8].tobytes() == np.ascontiguousarray(d["px"]["info"]).tobytes()
            worst["cost"] = max(worst["cost"], abs(d["px"]["mse"] - r["px"]["mse"]) / r["px"]["mse"])
            worst["grad10"] = max(worst["grad10"], _rel(d["grad10"], r["grad10"]))
            worst["info10"] = max(worst["info10"], _rel(d["info10"], r["info10"]))
            worst["grad"] = max(worst["grad"], _rel(d["px"]["grad"], r["px"]["grad"]))
            worst["info"] = max(worst["info"], _rel(d["px"]["info"], r["px"]["info"]))
        print(f"level {L}, K = 0, device vs host reference, worst relative difference:", {k: f"{v:.3e}" for k, v in worst.items()})
        bad += [(L, k, v) for k, v in worst.items() if not (v <= 1e-6 and v <= 10 * MEASURED_LIN[k])]
    assert not bad, bad


@pytest.mark.parametrize("name", list(R.ROWS))
def test_accuracy_rows_match_reference_and_truth(eng, rref, name):
    """an accuracy row (R.ROWS: exposure step 0.7 / +25, with and without the block, at one level and at four) on seeds 1, 2, 5, 11, in calls of n = 3
    and n = 1: at every level flags, trials, accepted, both valid counts and both outlier counts equal the host reference's; the final offsets lie within
    1e-4 px of the reference's and within the row's gate of the truth; hnet_op_photo_align_pyramid on the same pair, start and trials ends at least 3 x
    further from the truth (except R.RATIO_DROPPED)"""
    levels, kw = R.row_opts(name)
    gate = R.ROWS[name][4]
    i1, i2, truth, start = R.row_pairs(name)
    dout, dlv = _run_in_threes(eng, i1, i2, start, levels, **kw)
    rout, rlv = R.ref_run(rref, i1, i2, start, levels, **kw)
    old = np.concatenate([eng.op_photo_align_pyramid(i1[:3], i2[:3], start[:3], levels=levels, max_iterations=kw["max_iterations"]),
                          eng.op_photo_align_pyramid(i1[3:], i2[3:], start[3:], levels=levels, max_iterations=kw["max_iterations"])])
    for i, seed in enumerate(U.SEEDS):
        report = f"{name} seed {seed}\ndevice:\n{R.describe_levels(dlv[i], truth[i])}\nreference:\n{R.describe_levels(rlv[i], truth[i])}"
        assert dout[i].tobytes() == dlv[i, 0].tobytes()
        for L in range(levels):
            assert _trace(dlv[i, L]) == _trace(rlv[i, L]), report
        diff = float(np.abs(dout[i]["px"]["offsets_px"].astype(np.float64) - rout[i]["px"]["offsets_px"]).max())
        err = R.worst_px(dout[i], truth[i])
        err_old = float(np.abs(old[i]["offsets_px"].astype(np.float64) - truth[i]).max())
        print(f"{name} seed {seed}: {err:.4f} px from the truth (gate {gate:.4f}), {diff:.2e} px from the reference, without the model {err_old:.4f} px "
              f"({err_old / err:.1f} x), gain {dout[i]['gain']:.4f} (reference {rout[i]['gain']:.4f}), bias {dout[i]['bias']:.3f}")
        assert diff <= OFFSETS_VS_REFERENCE_PX, report
        assert err < gate, report
        assert abs(dout[i]["gain"] - rout[i]["gain"]) < 1e-6 and abs(dout[i]["bias"] - rout[i]["bias"]) < 1e-4, report
        if (name, seed) not in R.RATIO_DROPPED:
            assert err_old >= R.RATIO * err, report


def test_hostile_starts_on_device(eng, rref):
    """the hostile starts of the CPU test, model on, levels = 4, at K = 8 and K = 0, in calls of n = 3 and n = 1: the device's whole trace (flags,
    trials, accepted, counts, outlier counts) equals the host's at every level and the offsets lie within 1e-4 px (bit for bit where the level made
    no trial); the NaN keeps its payload"""
    cs = R.hostile_cases()
    for K1 in (K, 0):
        for lo in range(0, len(cs), 3):
            grp = cs[lo:lo + 3]
            by_opts = {}
            for c in grp:
                by_opts.setdefault(tuple(sorted(c[4].items())), []).append(c)
            for okey, members in by_opts.items():
                kw = dict(okey)
                i1, i2, start = np.stack([c[1] for c in members]), np.stack([c[2] for c in members]), np.stack([c[3] for c in members])
                out, dev = eng.op_photo_align_robust(i1, i2, start, levels=LEVELS, want_levels=True, max_iterations=K1, **kw)
                _, ref = R.ref_run(rref, i1, i2, start, LEVELS, max_iterations=K1, **kw)
                for b, c in enumerate(members):
                    name, flag = c[0], c[5]
                    for L in range(LEVELS):
                        d, r = dev[b, L], ref[b, L]
                        assert _trace(d) == _trace(r), (name, K1, L, _trace(d), _trace(r))
                        if flag is not None:
                            assert d["px"]["flags"] == flag and d["px"]["offsets_px"].tobytes() == r["px"]["offsets_px"].tobytes() == start[b].tobytes()
                        elif name != "nan":
                            assert np.abs(d["px"]["offsets_px"].astype(np.float64) - r["px"]["offsets_px"]).max() <= OFFSETS_VS_REFERENCE_PX, (name, L)
                        if name != "nan":
                            for f in ("gain", "bias", "grad10", "info10"):
                                assert np.isfinite(d[f]).all(), (name, L, f)
                        if flag in (U.DEGENERATE, U.FEW_PIXELS):
                            assert not d["info10"].any() and not d["grad10"].any() and d["px"]["mse0"] == 0.0
                    assert out[b].tobytes() == dev[b, 0].tobytes()
                    if name == "nan":
                        assert out[b]["px"]["offsets_px"].view(np.uint32)[3] == 0x7FC12345


@pytest.mark.parametrize("levels", [1, 4])
def test_model_off_is_the_pyramid_call(eng, levels):
    """brightness = 0 and huber_k = 0: the field px of every record of every level equals hnet_op_photo_align_pyramid's record on the same context byte for
    byte, n = 3 (a basin pair, a smooth pair from 0.75 px, a stock pair from its prior), 8 trials and none; gain / bias stay 1 / 0 and rows and
    columns 8, 9 of info10 are zero"""
    b, s, st = P.basin_pair(1, 32.0), U.smooth_pair(5, 8.0), U.stock_pair(2)
    i1, i2 = np.stack([b[0], s[0], st[0]]), np.stack([b[1], s[1], st[1]])
    start = np.stack([np.zeros(8, np.float32), np.full(8, 0.75, np.float32), st[3]])
    for K1 in (K, 0):
        want, wlv = eng.op_photo_align_pyramid(i1, i2, start, levels=levels, want_levels=True, max_iterations=K1)
        out, lv = eng.op_photo_align_robust(i1, i2, start, levels=levels, want_levels=True, max_iterations=K1, brightness=0, huber_k=0.0)
        assert np.ascontiguousarray(out["px"]).tobytes() == want.tobytes() and np.ascontiguousarray(lv["px"]).tobytes() == wlv.tobytes()
        assert (lv["gain"] == 1.0).all() and (lv["bias"] == 0.0).all() and not lv["n_outliers0"].any() and not lv["n_outliers"].any()
        assert not lv["info10"][:, :, 8:].any() and not lv["info10"][:, :, :, 8:].any() and not lv["grad10"][:, :, 8:].any()
        assert np.ascontiguousarray(lv["info10"][:, :, :8, :8]).tobytes() == np.ascontiguousarray(lv["px"]["info"]).tobytes()
    if levels == 1:
        assert np.ascontiguousarray(out["px"]).tobytes() == eng.op_photo_align(i1, i2, start, max_iterations=0).tobytes()


def test_batch_independence(eng):
    """a pair's `out` and `levels_out` bytes are the same alone, in slot 0 and in the last slot of n = 3, across two runs, and beside a pair that stops
    DEGENERATE at every level"""
    i1, i2, _, start = R.row_pairs("block-4levels")
    run = lambda idx, st=None: eng.op_photo_align_robust(i1[idx], i2[idx], start[idx] if st is None else st, levels=LEVELS, want_levels=True, max_iterations=K)
    o2, lv2 = run([2])                                                        # alone
    o0, lv0 = run([0])
    o, lv = run([2, 1, 0])                                                    # slot 0; pair 0 in the last slot of n = 3
    assert o[0].tobytes() == o2[0].tobytes() and lv[0].tobytes() == lv2[0].tobytes()
    assert o[2].tobytes() == o0[0].tobytes() and lv[2].tobytes() == lv0[0].tobytes()
    ob, lvb = run([2, 1, 0])                                                  # a second run
    assert ob.tobytes() == o.tobytes() and lvb.tobytes() == lv.tobytes()
    line = np.array([0, 0, 10, 5, 20, 10, 30, 15], np.float32) - np.array([0, 0, 0, 223, 319, 223, 319, 0], np.float32)
    o, lv = run([3, 2], np.stack([line, start[2]]))                           # beside a pair without a homography
    assert (lv[0]["px"]["flags"] == U.DEGENERATE).all() and (lv[0]["px"]["trials"] == 0).all()
    assert o[1].tobytes() == o2[0].tobytes() and lv[1].tobytes() == lv2[0].tobytes()


def test_sessions_call_is_read_only(blob, eng):
    """hnet_sessions_photo_align_robust on two sessions equals the operator call on the same frames byte for byte (out and levels_out); image counts,
    sequence numbers, times and hnet_sessions_last_timing stay as they were"""
    from cuahn_vio_amd import _capi
    from cuahn_vio_amd.homography_net import HnetEngine, HnetSessions
    i1, i2, _, start = R.row_pairs("block-4levels")
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=3)
    s = HnetSessions(e, 3)
    pick = [1, 3]
    s.push([0, 2], i1[pick], t=[1.0, 1.0])
    s.push([0, 2], i2[pick], t=[2.0, 2.0])
    s.push([1], i1[:1], t=[1.0])
    s.set_seq(2, 41)
    s.infer([2, 0], np.zeros((2, 8)))                                         # (so that last_timing holds something)
    state = lambda: ([s.image_count(i) for i in range(3)], [s.seq(i) for i in range(3)], [s.latest_time(i) for i in range(3)], s.last_timing())
    before = state()
    ids = np.array([2, 0], np.int32)                                          # session 2 holds pair 3, session 0 pair 1
    out, lv = s.photo_align_robust(ids, start[:2], levels=LEVELS, want_levels=True, max_iterations=K)
    assert state() == before and e.last_photo_align_device_ms() > 0.0
    want, wlv = eng.op_photo_align_robust(i1[[3, 1]], i2[[3, 1]], start[:2], levels=LEVELS, want_levels=True, max_iterations=K)
    assert out.tobytes() == want.tobytes() and lv.tobytes() == wlv.tobytes()
    for bad, status in (([0, 1], NOT_READY), ([0, 0], INVALID), ([3], INVALID)):
        with pytest.raises(_capi.HnetError) as ei:
            s.photo_align_robust(bad, np.zeros((len(bad), 8), np.float32))
        assert ei.value.status == status, bad
    for kw in (dict(levels=5), dict(huber_k=-1.0), dict(brightness=0, gain0=2.0)):
        with pytest.raises(_capi.HnetError) as ei:
            s.photo_align_robust(ids, start[:2], **kw)
        assert ei.value.status == INVALID and state() == before
    s.close()
    e.close()


def test_refusals_write_nothing(eng):
    """levels 0 and 5, a NULL out, NULL frames, NULL options, n = 0, n above max_batch (3) and every refused option return the documented code and leave
    `out` and `levels_out` untouched; a legal call writes its own records and nothing behind them"""
    from cuahn_vio_amd import _capi
    L = _capi.lib()
    size = _capi.PHOTO_ROBUST_DTYPE.itemsize
    i1, i2, _, _ = R.row_pairs("gain-4levels")
    out, lvo = np.full(4 * size, 0xA5, np.uint8), np.full(4 * 4 * size, 0x5A, np.uint8)
    keep, keep_lv = out.copy(), lvo.copy()
    a, b = np.ascontiguousarray(i1), np.ascontiguousarray(i2)
    x0 = np.zeros((4, 8), np.float32)
    ok = _capi.photo_robust_opts()

    def call(n, o, levels=4, img1=a.ctypes.data, outp=out.ctypes.data):
        return L.hnet_op_photo_align_robust(eng.handle, img1, b.ctypes.data, n, x0.ctypes.data, C.addressof(o) if o is not None else None, levels, outp,
                                            lvo.ctypes.data)
    assert call(1, ok, levels=0) == INVALID and call(1, ok, levels=5) == INVALID and call(1, ok, levels=-1) == INVALID
    assert call(1, ok, outp=None) == INVALID and call(1, ok, img1=None) == INVALID and call(1, None) == INVALID and call(0, ok) == INVALID
    assert call(4, ok) == CAPACITY
    nan, inf = float("nan"), float("inf")
    for kw in (dict(max_iterations=33), dict(min_valid=-1), dict(lambda0=1.0000001e100), dict(eps_px=-1.0), dict(brightness=2), dict(brightness=-1),
               dict(huber_k=-1.0), dict(huber_k=nan), dict(huber_k=inf), dict(gain0=0.0), dict(gain0=-1.0), dict(gain0=nan), dict(gain0=inf),
               dict(bias0=nan), dict(bias0=-inf), dict(brightness=0, gain0=1.5), dict(brightness=0, bias0=-1.0)):
        assert call(1, _capi.photo_robust_opts(**kw)) == INVALID, kw
    assert out.tobytes() == keep.tobytes() and lvo.tobytes() == keep_lv.tobytes()
    assert call(1, _capi.photo_robust_opts(max_iterations=1), levels=4) == 0                                    # (a legal call does write both)
    assert out[:size].tobytes() != keep[:size].tobytes() and out[size:].tobytes() == keep[size:].tobytes()
    assert lvo[:4 * size].tobytes() != keep_lv[:4 * size].tobytes() and lvo[4 * size:].tobytes() == keep_lv[4 * size:].tobytes()
