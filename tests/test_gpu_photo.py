"""Photometric residual records on the device (include/hnet.h hnet_photo_residual; csrc/kernels_photo.hip): the operator call against the
existing device warp and the host reference, shapes and bitwise independence of the batch, the reference model's recorded sums, the sessions call, and
the records of hnet_filters_step / _advance against the operator call on the same frames and candidates.  Main model prior-3, N = 16."""
import ctypes as C
import os

import numpy as np
import pytest

import test_gpu_filters as tg
import test_gpu_filters_innov as ti
import test_sessions_iterative_cpu as ic
from conftest import load_case
from test_photo_cpu import build_photo_ref, photo_ref_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPIX = 224 * 320
P4 = np.array([0, 0, 0, 223, 319, 223, 319, 0], np.float32)
INVALID, NOT_READY, CAPACITY = 1, 4, 5
PREC_BF16X3, PREC_F16X2 = 2, 3


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return build_photo_ref(tmp_path_factory.mktemp("photo_ref_gpu"))


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=8)
    yield e
    e.close()


def _corner_offsets(h):
    """the four-corner offsets of a 3 x 3 homography: where it takes the image corners, minus the corners"""
    h = np.asarray(h, np.float64).reshape(3, 3)
    out = np.zeros(8)
    for c in range(4):
        x = h @ np.array([P4[2 * c], P4[2 * c + 1], 1.0])
        out[2 * c:2 * c + 2] = x[:2] / x[2] - P4[2 * c:2 * c + 2]
    return out.astype(np.float32)


def _pairs(rng, n):
    """n textured pairs: a random frame and a shifted, brightened copy of it"""
    a = rng.integers(0, 256, (n, 224, 320), dtype=np.uint8)
    b = np.stack([np.roll(a[i], (i % 5 - 2, i % 7 - 3), axis=(0, 1)) for i in range(n)])
    return a, (b // 2 + 40).astype(np.uint8)


def _cands(priors, net):
    """the filters' candidates [n, 2 + iters, 8]: zero, the fp32 prior of iteration 0, the packed mean of every forward"""
    iters, n = net.shape[0], net.shape[1]
    return np.concatenate([np.zeros((n, 1, 8), np.float32), priors[0][:, None, :], np.transpose(net[:, :, :8], (1, 0, 2))], axis=1).reshape(n, 2 + iters, 8)


def _session_frames(s, ids):
    return np.stack([s.frame(int(i), 0) for i in ids]), np.stack([s.frame(int(i), 1) for i in ids])


def test_operator_matches_device_warp_and_reference(eng, pref):
    """a. n = 3, m = 4 (identity, shift, out of bounds, perspective: the homographies of warp_s11.npz as corner offsets): the map equals
    |op_warp(f2, op_dlt(p4 + off)) - f1| * 255 exactly; sum is the float64 sum of the map within the summation-order bound 1e-10; sum_inside and n_inside
    agree with the host reference up to the pixels on the inside bound"""
    from cuahn_vio_amd import synth
    from oracle import pyoracle
    g = np.load(os.path.join(ROOT, "tests", "golden", "warp_s11.npz"))
    off = np.stack([_corner_offsets(g["H_" + k]) for k in ("identity", "shift", "oob", "persp")])
    assert not off[0].any()
    pairs = [synth.make_pair(s)[:2] for s in (11, 1, 2)]
    i1, i2 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    offs = np.repeat(off[None], 3, 0)
    rec, emap = eng.op_photo_residual(i1, i2, offs, want_map=True)
    ref, edge = photo_ref_records(pref, i1, i2, offs)
    hs = eng.op_dlt((P4[None] + off).astype(np.float32))
    worst = {"sum_vs_map": 0.0, "dn": 0, "dsum_inside": 0.0}
    for b in range(3):
        f1, f2 = pyoracle.as_f32_image(i1[b]), pyoracle.as_f32_image(i2[b])
        for c in range(4):
            want = np.abs(eng.op_warp(f2, hs[c]) - f1) * np.float32(255)
            assert want.dtype == np.float32 and emap[b, c].tobytes() == want.tobytes(), (b, c)
            r = rec[b, c]
            msum = float(emap[b, c].astype(np.float64).sum())
            worst["sum_vs_map"] = max(worst["sum_vs_map"], abs(r["sum"] - msum) / msum)
            dn = abs(int(r["n_inside"]) - int(ref["n_inside"][b, c]))
            ds = abs(r["sum_inside"] - ref["sum_inside"][b, c])
            worst["dn"], worst["dsum_inside"] = max(worst["dn"], dn), max(worst["dsum_inside"], ds)
            assert r["flags"] == 0
            assert abs(r["sum"] - msum) <= 1e-10 * msum
            assert dn <= edge[b, c], (b, c, dn, edge[b, c])
            assert ds <= 255.0 * dn + 1e-6 * r["sum"], (b, c, ds, dn)
        assert rec[b, 0]["n_inside"] == NPIX and rec[b, 0]["sum"] == rec[b, 0]["sum_inside"]
        assert rec[b, 2]["n_inside"] < rec[b, 1]["n_inside"] < NPIX
    print(f"operator: |sum - sum(map)| / sum <= {worst['sum_vs_map']:.2e}; vs host reference: |d n_inside| <= {worst['dn']}, "
          f"|d sum_inside| <= {worst['dsum_inside']:.3e}; n_edge {edge.tolist()}")
    plain = eng.op_photo_residual(i1, i2, offs)                              # without the map: the same records
    assert plain.tobytes() == rec.tobytes()


def test_shapes_and_batch_independence(blob, eng):
    """b. (n, m) = (1, 1), (2, 66), (8, 3) and n = 9 at max_batch 9; a pair's record is bitwise the same alone, in slot 0, in the last slot and across runs;
    and the operator call's refusals"""
    from cuahn_vio_amd import _capi
    from cuahn_vio_amd.homography_net import HnetEngine
    rng = np.random.default_rng(5)
    a, b = _pairs(rng, 9)
    off = (rng.standard_normal((9, 66, 8)) * 8).astype(np.float32)
    off[:, 0] = 0
    alone = [eng.op_photo_residual(a[i], b[i], off[i:i + 1]) for i in range(9)]          # (1, 66) each
    assert alone[0][:, :1].tobytes() == eng.op_photo_residual(a[0], b[0], off[0:1, :1]).tobytes()      # (1, 1)
    two = eng.op_photo_residual(a[[3, 0]], b[[3, 0]], off[[3, 0]])                        # (2, 66): pair 0 last, pair 3 first
    assert two[0].tobytes() == alone[3][0].tobytes() and two[1].tobytes() == alone[0][0].tobytes()
    eight = eng.op_photo_residual(a[:8], b[:8], off[:8, :3])                              # (8, 3)
    for i in range(8):
        assert eight[i].tobytes() == alone[i][0, :3].tobytes(), i
    order = [7, 1, 2, 3, 4, 5, 6, 0]                                                       # pair 0 in the last slot, pair 7 in slot 0
    perm = eng.op_photo_residual(a[order], b[order], off[order, :3])
    assert perm[7].tobytes() == eight[0].tobytes() and perm[0].tobytes() == eight[7].tobytes()
    assert eng.op_photo_residual(a[:8], b[:8], off[:8, :3]).tobytes() == eight.tobytes()   # a second run
    assert np.all(eight["flags"] == 0) and np.all(eight["n_inside"][:, 0] == NPIX) and np.all(np.isfinite(eight["sum"]))
    e9 = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=9)
    nine = e9.op_photo_residual(a, b, off[:, :3])
    for i in range(9):
        assert nine[i].tobytes() == alone[i][0, :3].tobytes(), i
    e9.close()
    # refusals write nothing
    L = _capi.lib()
    out = np.zeros((9, 67), _capi.PHOTO_RESIDUAL_DTYPE)
    offs = np.zeros((9, 67, 8), np.float32)
    args = lambda n, m: (eng.handle, a.ctypes.data, b.ctypes.data, n, offs.ctypes.data_as(C.POINTER(C.c_float)), m, out.ctypes.data, None)
    assert L.hnet_op_photo_residual(*args(9, 3)) == CAPACITY
    assert L.hnet_op_photo_residual(*args(0, 3)) == INVALID and L.hnet_op_photo_residual(*args(1, 0)) == INVALID
    assert L.hnet_op_photo_residual(*args(1, 67)) == INVALID
    assert not out["sum"].any() and not out["n_inside"].any()


@pytest.mark.parametrize("name", ["full_p0_s1", "prior3_pm30_s28", "traj_pair40_prior3"])
def test_golden_pin_on_device(eng, name):
    """c. the device record of the golden's mean64 carries the reference model's own error sum"""
    g, i1, i2, _prior, _btr = load_case(name)
    rec = eng.op_photo_residual(i1, i2, g["mean64"])
    rel = abs(rec["sum"][0, 0] - g["err_stats64"][0]) / g["err_stats64"][0]
    print(f"{name}: device sum {rec['sum'][0, 0]:.6f} vs err_stats64 {g['err_stats64'][0]:.6f}: {rel:.2e}")
    assert rel < 2e-5


def test_sessions_call_is_read_only(blob, eng):
    """d. the records equal the operator call on hnet_sessions_get_frame's two frames, bitwise; counts, sequence numbers, times and last_timing are
    untouched; a one-image session and a repeated id are refused as by hnet_sessions_infer"""
    from cuahn_vio_amd import _capi
    e, s, f = tg._setup(blob, 5, 1)
    rng = np.random.default_rng(8)
    s.reset(4)
    s.push([4], tg._frames(rng, 1), t=[9.0])
    ids = np.array([3, 0, 2], np.int32)
    s.set_seq(3, 41)
    pr = rng.standard_normal((3, 8)) * 3
    s.infer(ids, pr)                                                         # (so that last_timing holds something)
    before = ([s.image_count(i) for i in range(5)], [s.seq(i) for i in range(5)], [s.latest_time(i) for i in range(5)], s.last_timing())
    off = (rng.standard_normal((3, 5, 8)) * 6).astype(np.float32)
    rec = s.photo_residual(ids, off)
    prev, curr = _session_frames(s, ids)
    assert rec.tobytes() == eng.op_photo_residual(prev, curr, off).tobytes()
    assert (prev != curr).any() and np.all(rec["flags"] == 0)
    after = ([s.image_count(i) for i in range(5)], [s.seq(i) for i in range(5)], [s.latest_time(i) for i in range(5)], s.last_timing())
    assert before == after
    for bad, status in (([3, 4], NOT_READY), ([3, 3], INVALID), ([5], INVALID), (list(range(5)) * 2, CAPACITY)):
        with pytest.raises(_capi.HnetError) as ei:
            s.photo_residual(bad, np.zeros((len(bad), 1, 8), np.float32))
        assert ei.value.status == status, bad
    for o in (f, s, e):
        o.close()


@pytest.mark.parametrize("iters", [1, 3])
def test_filters_step_records(blob, eng, iters):
    """e. 8 sessions, windows of 0 - 40 intervals: last_photometric equals, bitwise, the operator call on the sessions' frames with the candidates
    [0, last_priors[0], net_out[it][:, :8]]"""
    _capi, _, _, HnetFilters = tg._mods()
    n = 8
    e, s, f = tg._setup(blob, n, iters)
    L = _capi.lib()
    none = np.zeros((n, 2 + iters), _capi.PHOTO_RESIDUAL_DTYPE)
    assert L.hnet_filters_last_photometric(f._f, n, none.ctypes.data) == INVALID and not none["sum"].any()      # before enabling
    f.enable_photometric()
    assert L.hnet_filters_enable_photometric(f._f) == INVALID                # once per object
    assert L.hnet_filters_last_photometric(f._f, n, none.ctypes.data) == INVALID                                 # no step yet
    t_frame = 1.0 + 0.1 * 11
    ps, sts, imus = ti._inputs(_capi, HnetFilters, 70 + iters, n, t_frame, [0, 1, 2, 16, 40, 16, 3, 7])
    ti._load(f, s, ps, sts)
    ids = np.arange(n, dtype=np.int32)
    out, net, upd = f.step(ids, [t_frame] * n, imus)
    rec = f.last_photometric(n)
    prev, curr = _session_frames(s, ids)
    cands = _cands(f.last_priors(n), net)
    want = eng.op_photo_residual(prev, curr, cands)
    res = rec["sum_inside"] / np.maximum(rec["n_inside"], 1)
    print(f"step, iters {iters}: mean inside residual identity {res[:, 0].mean():.3f}, prior {res[:, 1].mean():.3f}, estimates {res[:, 2:].mean(axis=0).tolist()}; "
          f"bitwise equal to the operator call: {rec.tobytes() == want.tobytes()}")
    assert rec.shape == (n, 2 + iters) and rec.tobytes() == want.tobytes()
    assert np.all(rec["n_inside"][:, 0] == NPIX) and np.all(rec["flags"] == 0)
    assert rec.tobytes() != eng.op_photo_residual(curr, prev, cands).tobytes()                # (swapped frames would show)
    assert len({rec[:, k].tobytes() for k in range(2 + iters)}) == 2 + iters                   # (and so would a repeated candidate)
    with pytest.raises(_capi.HnetError) as ei:
        f.last_photometric(n - 1)
    assert ei.value.status == INVALID
    for o in (f, s, e):
        o.close()


def test_off_path_step(blob):
    """f. with photometric records enabled a step computes the states, network outputs, priors, updates and sequence numbers of an object without them, bit
    for bit; with innovations enabled too, in either order, both kinds of records are those of the objects with one feature"""
    _capi, _, _, HnetFilters = tg._mods()
    n, iters = 8, 3
    objs = {k: tg._setup(blob, n, iters) for k in ("none", "photo", "innov", "photo_innov", "innov_photo")}
    objs["photo"][2].enable_photometric()
    objs["innov"][2].enable_innovations()
    objs["photo_innov"][2].enable_photometric(); objs["photo_innov"][2].enable_innovations()
    objs["innov_photo"][2].enable_innovations(); objs["innov_photo"][2].enable_photometric()
    t_frame = 1.0 + 0.1 * 11
    ps, sts, imus = ti._inputs(_capi, HnetFilters, 81, n, t_frame, [0, 1, 2, 16, 40, 16, 3, 7])
    ids = np.arange(n, dtype=np.int32)
    res = {}
    for k, (e, s, f) in objs.items():
        ti._load(f, s, ps, sts, seq=7)
        res[k] = f.step(ids, [t_frame] * n, imus)
    base = res["none"]
    for k, (e, s, f) in objs.items():
        assert all(x.tobytes() == y.tobytes() for x, y in zip(res[k], base)), k
        assert f.last_priors(n).tobytes() == objs["none"][2].last_priors(n).tobytes(), k
        assert f.get_state(ids).tobytes() == objs["none"][2].get_state(ids).tobytes(), k
        assert [s.seq(int(i)) for i in ids] == [7 + iters] * n, k
    photo = objs["photo"][2].last_photometric(n)
    innov = objs["innov"][2].last_innovations(n)
    for k in ("photo_innov", "innov_photo"):
        assert objs[k][2].last_photometric(n).tobytes() == photo.tobytes(), k
        assert objs[k][2].last_innovations(n).tobytes() == innov.tobytes(), k
    assert np.all(innov["flag"] == ti.USED) and np.all(photo["n_inside"][:, 0] == NPIX)
    L = _capi.lib()
    scratch = photo.copy()
    for k in ("none", "innov"):                                               # the last call ran without the feature
        assert L.hnet_filters_last_photometric(objs[k][2]._f, n, scratch.ctypes.data) == INVALID
    for e, s, f in objs.values():
        for o in (f, s, e):
            o.close()


def test_off_path_and_subsets_advance(blob, eng):
    """f, g. three advances on rings of 64 readings that wrap: everything an advance returns equals that of an object without the records, and of one
    with innovations too; then a call in which only sessions 6, 1, 3 (in that order) have a new frame has records for exactly those, in listed order,
    equal to the operator call; and a call in which nothing steps has none"""
    _capi, _, _, HnetFilters = tg._mods()
    iters = 3
    objs = [tg._setup(blob, 8, iters) for _ in range(3)]                      # none | photometric | innovations, then photometric
    objs[1][2].enable_photometric()
    objs[2][2].enable_innovations(); objs[2][2].enable_photometric()
    for _e, _s, f in objs:
        f.enable_feed(64)
    rng = np.random.default_rng(29)
    counts = [0, 1, 2, 16, 40, 16, 3, 7]
    ids = np.arange(8, dtype=np.int32)
    t_frame = np.full(8, 1.0 + 0.1 * 11)
    ps, hist, fed = [], [], [0] * 8
    for i in range(8):
        p = tg._params(HnetFilters, rng, i)
        st = tg._state(_capi, rng, t_frame[i])
        for _e, _s, f in objs:
            f.set_params(i, p)
            f.set_state(i, st)
        ps.append(p)
        ts = t_frame[i] + p.cam_imu_dt - 0.0007 + 0.002 * np.arange(4 * 42 + 4)
        r = np.zeros(len(ts), _capi.IMU_DTYPE)
        r["t"], r["wm"], r["am"] = ts, rng.standard_normal((len(ts), 3)) * 0.3, rng.standard_normal((len(ts), 3)) * 0.5 + [0, 0, 9.81]
        hist.append(r)
    fr = tg._frames(rng, 4)

    def feed(sub):
        chunks = []
        for i in sub:
            upto = int(np.searchsorted(hist[i]["t"], t_frame[i] + ps[i].cam_imu_dt, side="right")) + 1
            chunks.append(hist[i][fed[i]:upto])
            fed[i] = upto
        for _e, _s, f in objs:
            f.feed_imu(np.asarray(sub, np.int32), chunks)

    for tick in range(3):
        t_frame = t_frame + 0.002 * np.maximum(counts, 0.1) + 0.0004
        for _e, s, _f in objs:
            s.push(ids, np.repeat(fr[tick][None], 8, 0), t=list(t_frame))
        feed(range(8))
        res = [f.advance(ids) for _e, _s, f in objs]
        assert list(res[0][3]) == [_capi.ADV_STEPPED] * 8 and list(res[0][2]) == [iters] * 8
        for k in (1, 2):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(res[k], res[0])), (tick, k)
            assert objs[k][2].last_priors(8).tobytes() == objs[0][2].last_priors(8).tobytes()
            assert objs[k][2].get_state(ids).tobytes() == objs[0][2].get_state(ids).tobytes()
            assert [objs[k][1].seq(int(i)) for i in ids] == [objs[0][1].seq(int(i)) for i in ids]
        rec = objs[1][2].last_photometric(8)
        assert rec.tobytes() == objs[2][2].last_photometric(8).tobytes()
        prev, curr = _session_frames(objs[1][1], ids)
        assert rec.tobytes() == eng.op_photo_residual(prev, curr, _cands(objs[1][2].last_priors(8), res[1][1])).tobytes(), tick
    assert max(fed) > 64                                                      # the rings wrapped
    # g. only sessions 6, 1, 3 get a new frame; all 8 are listed, those three in the order 6, 1, 3
    sub = [6, 1, 3]
    for i in sub:
        t_frame[i] += 0.002 * max(counts[i], 0.1) + 0.0004
    for _e, s, _f in objs:
        s.push(np.asarray(sub, np.int32), np.repeat(fr[3][None], 3, 0), t=[t_frame[i] for i in sub])
    feed(sub)
    listed = np.array([6, 0, 1, 2, 3, 4, 5, 7], np.int32)
    e, s, f = objs[1]
    out, net, upd, status = f.advance(listed)
    stepped = [int(i) for i, st in zip(listed, status) if st == _capi.ADV_STEPPED]
    assert stepped == sub and all(st == _capi.ADV_NO_FRAME for i, st in zip(listed, status) if int(i) not in sub)
    rec = f.last_photometric(3)
    rows = [int(np.where(listed == i)[0][0]) for i in sub]
    prev, curr = _session_frames(s, sub)
    assert rec.tobytes() == eng.op_photo_residual(prev, curr, _cands(f.last_priors(3), net[:, rows, :])).tobytes()
    L = _capi.lib()
    assert L.hnet_filters_last_photometric(f._f, 8, np.zeros((8, 2 + iters), _capi.PHOTO_RESIDUAL_DTYPE).ctypes.data) == INVALID
    # nothing steps: no records
    out, net, upd, status = f.advance(listed)
    assert all(st == _capi.ADV_NO_FRAME for st in status)
    keep = np.zeros((3, 2 + iters), _capi.PHOTO_RESIDUAL_DTYPE)
    assert L.hnet_filters_last_photometric(f._f, 3, keep.ctypes.data) == INVALID and not keep["sum"].any()
    for e, s, f in objs:
        for o in (f, s, e):
            o.close()


def test_repeat_recomputes_records(blob):
    """h. an iterative model whose activations overflow the fp16 planes (the set-up of test_gpu_filters_innov.py d): the step demotes it once and reruns; the
    records are those of fresh objects whose iterative engine runs HNET_PREC_BF16X3 from the start, bit for bit"""
    from cuahn_vio_amd.homography_net import HnetEngine
    _capi, _, _, HnetFilters = tg._mods()
    iters, n = 3, 4
    ov = ic.overflow_iterative_blob()
    t_frame = 1.0 + 0.1 * 11
    ps, sts, imus = ti._inputs(_capi, HnetFilters, 47, n, t_frame, [16])
    ids = np.arange(n, dtype=np.int32)
    res = []
    for prec in (PREC_F16X2, PREC_BF16X3):
        e, s, f = tg._setup(blob, n, iters, precision=PREC_F16X2)
        ie = HnetEngine(ov, variant="prior1", mc_samples=8, dropout_p=0.1, mc_seed=9, max_batch=8, precision=prec)
        s.set_iterative_model(ie)
        f.enable_photometric()
        ti._load(f, s, ps, sts)
        out, net, upd = f.step(ids, [t_frame] * n, imus)
        rec = f.last_photometric(n)
        assert ie.precision() == PREC_BF16X3 and e.precision() == PREC_F16X2   # (demoted once, the iterative context only)
        assert np.all(np.isfinite(net)) and np.all(np.isfinite(rec["sum"])) and np.all(rec["flags"] == 0)
        res.append((out, net, upd, rec))
        for o in (f, s, ie, e):
            o.close()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(res[0], res[1]))
