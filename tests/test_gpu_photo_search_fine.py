"""The fine stage of the search around the oriented winner on the device (include/hnet.h hnet_op_photo_search_fine, hnet_sessions_photo_search_fine;
csrc/kernels_photo_search_fine.hip) against the host reference tests/cpp/photo_search_fine_ref.cpp, byte for byte: the warp and the sums are
integers and the score is three correctly rounded double operations, so there is no tolerance anywhere in this file but the distance of a start from the
truth.  Sessions objects of 4 cameras on a context of max_batch 8."""
import ctypes as C

import numpy as np
import pytest

import photo_search_fine_util as F
import photo_search_oriented_util as O
import photo_search_util as S
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, CAPACITY = 1, 4, 5
N_CAM = 4


@pytest.fixture(scope="module")
def fref(tmp_path_factory):
    return F.build_ref(tmp_path_factory.mktemp("photo_search_fine_ref_gpu"))


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=8)
    yield e
    e.close()


@pytest.fixture
def fleet(eng):
    from cuahn_vio_amd.homography_net import HnetSessions
    made = []

    def make():
        s = HnetSessions(eng, N_CAM)
        made.append(s)
        return s
    yield make
    for s in made:
        s.close()


def _same(dev, sc, ref, rsc):
    keys = ["flags", "j", "ex", "ey", "sx", "sy", "score"]
    assert dev.tobytes() == ref.tobytes(), (dev["fine"][keys], ref["fine"][keys], dev["coarse"][["hyp", "n_scored"]], ref["coarse"][["hyp", "n_scored"]])
    assert sc.shape == rsc.shape and sc.tobytes() == rsc.tobytes()


def _run(eng, fref, a, b, o, hyps, fo, fine):
    """the device call and the host reference, equal byte for byte; the coarse part is hnet_op_photo_search_oriented's -> the device records"""
    ref, rsc = F.ref_run(fref, a, b, o, hyps, fo, fine)
    dev, sc = eng.op_photo_search_fine(a, b, hyps=hyps, fine=fine, fine_opts=F.fine_kw(fo), want_scores=True, **S.search_kw(o))
    _same(dev, sc, ref, rsc)
    assert eng.op_photo_search_fine(a, b, hyps=hyps, fine=fine, fine_opts=F.fine_kw(fo), **S.search_kw(o)).tobytes() == ref.tobytes()      # without the tables
    assert dev["coarse"].tobytes() == eng.op_photo_search_oriented(a, b, hyps=hyps, **S.search_kw(o)).tobytes()
    return dev


def test_tables_and_defaults_are_the_header_s(fref):
    """hnet_photo_search_fine_yaw_table gives the host reference's entries and _default_opts its bytes; fine = None builds the table that matches hyps.
    The library and the reference are built by two compilers, of which one may call sincos where the other calls sin and cos: a is compared to one unit
    in the last place and b to one step, and the middle column against the same library's coarse table byte for byte.  (Every other test of this file
    hands ONE table to the device and to the reference.)"""
    for first, step, count, n_fine in ((-180.0, 6.0, 60, 5), (-180.0, 12.0, 30, 5), (-36.0, 6.0, 13, 2), (0.0, 5.625, 64, 9)):
        t, r = _capi.photo_search_fine_yaw_table(first, step, count, n_fine), F.fine_yaw_table(fref, first, step, count, n_fine)
        assert t.shape == r.shape and (np.abs(t["a"] - r["a"]) <= np.spacing(1.0)).all() and np.abs(t["b"] - r["b"]).max() <= 1
        if n_fine % 2:
            assert t[:, n_fine // 2].tobytes() == _capi.photo_search_yaw_table(first, step, count).tobytes()
    assert _capi.photo_search_fine_table(None, None, 5).tobytes() == _capi.photo_search_fine_yaw_table().tobytes()
    t = _capi.photo_search_fine_table(None, O.yaw_table(fref, -180.0, 12.0, 30), 5)
    assert t.shape == (30, 5) and t[:, 2].tobytes() == O.yaw_table(fref, -180.0, 12.0, 30).tobytes()
    assert np.abs(t["a"] - F.fine_yaw_table(fref, -180.0, 12.0, 30, 5)["a"]).max() < 1e-12
    assert bytes(_capi.photo_search_fine_opts()) == bytes(F.fine_opts(fref))
    with pytest.raises(ValueError):
        _capi.photo_search_fine_yaw_table(0.0, 1.0, 65, 5)
    with pytest.raises(ValueError):
        _capi.photo_search_fine_yaw_table(0.0, 1.0, 4, 10)


@pytest.mark.parametrize("seed", S.SEEDS)
def test_one_pair_one_entry_radius_0(eng, fref, seed):
    """n = 1 with n_hyp = 1, n_fine = 1, r = 0: one shift is scored, the one at twice the coarse shift"""
    key, views, _, _ = S.cases(seed)
    ident = O.table(fref, *O.IDENTITY)
    fo = F.fine_opts(fref, n_fine=1, radius=0)
    dev = _run(eng, fref, key[None], views[seed % 4][None], S.search_opts(), ident, fo, ident.reshape(1, 1))
    p, c = dev[0]["fine"], dev[0]["coarse"]["base"]
    assert c["flags"] == _capi.PS_FOUND and p["flags"] == _capi.PSF_REFINED and (p["j"], p["ex"], p["ey"], p["sx"], p["sy"]) == (0, 0, 0, 2 * c["dx"], 2 * c["dy"])


@pytest.mark.parametrize("seed", S.SEEDS)
def test_three_pairs_in_two_slot_orders(eng, fref, seed):
    """n = 3 in two slot orders with a 5-entry table that holds a quarter turn and scaled entries and n_fine = 3: every record and the whole score table
    equal the host reference byte for byte; a pair's bytes are the same in any slot"""
    key, views, _ = O.yawed(seed)
    _, _, _, other = S.cases(seed)
    a, b = np.stack([key] * 4), np.concatenate([views[:3], other[None]])
    hyps, fo = O.table(fref, *O.TABLE5), F.fine_opts(fref, n_fine=3, radius=3)
    fine = F.fine_rows(fref, *F.around(O.TABLE5, 3, 6.0))
    for order in ([0, 3, 2], [2, 1, 0]):
        _run(eng, fref, a[order], b[order], S.search_opts(), hyps, fo, fine)


def test_64_by_9_entries_radius_4(eng, fref):
    """n = 1 with 64 x 9 entries and r = 4: all 81 shifts of all 9 entries, two passes of the workgroup"""
    key, views, poses = O.yawed(5)
    hyps, fine = O.yaw_table(fref, -180.0, 5.625, 64), F.fine_yaw_table(fref, -180.0, 5.625, 64, 9)
    dev = _run(eng, fref, key[None], views[1:2], S.search_opts(), hyps, F.fine_opts(fref, n_fine=9, radius=4), fine)
    assert dev["coarse"]["n_scored"][0] == 64 and dev["fine"]["flags"][0] == _capi.PSF_REFINED
    assert S.worst_px(dev["fine"]["start_px"][0], poses[1]) < S.worst_px(dev["coarse"]["base"]["start_px"][0], poses[1])


@pytest.mark.parametrize("seed", S.SEEDS)
def test_the_yawed_views_under_the_12_degree_table(eng, fref, seed):
    """the five yawed views of a seed under (30 x 12 degrees, n_fine 5, r 3): byte for byte the host reference, so the rows give its figures: every row
    REFINED, the fine start closer to the truth than the coarse one and inside the gate of photo_search_fine_util"""
    key, views, poses = O.yawed(seed)
    hyps, fine = O.yaw_table(fref, *F.TABLE_30), F.fine_yaw_table(fref, *F.TABLE_30, 5)
    dev = _run(eng, fref, np.stack([key] * len(views)), views, S.search_opts(), hyps, F.fine_opts(fref), fine)
    for i in range(len(views)):
        ec, ef = S.worst_px(dev["coarse"]["base"]["start_px"][i], poses[i]), S.worst_px(dev["fine"]["start_px"][i], poses[i])
        print(f"seed {seed} yaw {O.YAW_ROWS[i][0]:6.1f}: coarse start {ec:.2f} px, fine start {ef:.2f} px (gate {F.GATE_FINE_30:.2f})")
        assert dev["fine"]["flags"][i] == _capi.PSF_REFINED and ef < ec and ef <= F.GATE_FINE_30 < O.BASIN_PX
    auto = eng.op_photo_search_fine(np.stack([key] * len(views)), views, hyps=hyps)      # fine = None: the matching table (angles recovered from hyps), the defaults
    assert auto["coarse"].tobytes() == dev["coarse"].tobytes() and np.array_equal(auto["fine"][["flags", "j", "ex", "ey"]], dev["fine"][["flags", "j", "ex", "ey"]])
    assert np.abs(auto["fine"]["start_px"] - dev["fine"]["start_px"]).max() < 1e-3


@pytest.mark.parametrize("name", sorted(F.hand_built()))
def test_hand_built_cases_alone(eng, fref, name):
    """each hand-built case as frames of constant 4 x 4 blocks, with its own options and tables: byte for byte the host reference"""
    a, b, o, hyps, fo, fine = F.case_tables(fref, name)
    dev = _run(eng, fref, a[None], b[None], o, hyps, fo, fine)
    want = {"peak(30,20)": _capi.PSF_REFINED, "same-fine-entry-twice": _capi.PSF_REFINED, "tie-between-shifts": _capi.PSF_REFINED,
            "coarse-low-score": _capi.PSF_SKIPPED, "scale-half-scores-nothing": _capi.PSF_NOTHING_SCORED, "min-score-one": _capi.PSF_LOW_SCORE}
    assert dev["fine"]["flags"][0] == want[name]


def test_hand_built_cases_together(eng, fref):
    """the hand-built cases in one call of 6 under one set of options and one fine row that holds a scale-0.5 entry and the same entry twice"""
    h = F.hand_built()
    names = sorted(h)
    a, b = np.stack([F.expand4(h[n][0]) for n in names]), np.stack([F.expand4(h[n][1]) for n in names])
    hyps, fo = O.table(fref, *O.IDENTITY), F.fine_opts(fref, n_fine=3, radius=4, min_score=0.5)
    fine = F.fine_rows(fref, ((0.0, 0.5), (0.0, 1.0), (0.0, 1.0)))
    dev = _run(eng, fref, a, b, S.search_opts(min_overlap=16, min_score=0.5), hyps, fo, fine)
    got = dict(zip(names, dev))
    assert got["coarse-low-score"]["fine"]["flags"] == _capi.PSF_SKIPPED and np.array_equal(got["coarse-low-score"]["fine"]["start_px"].view(np.uint32), F.NAN32)
    p = got["peak(30,20)"]["fine"]
    assert (p["flags"], p["j"], p["sx"], p["sy"]) == (_capi.PSF_REFINED, 1, 60, 40)
    p = got["tie-between-shifts"]["fine"]
    assert (p["flags"], p["j"], p["ex"], p["ey"]) == (_capi.PSF_REFINED, 1, -1, 0)


def test_sessions_call(eng, fleet, fref):
    """hnet_sessions_photo_search_fine on the (prev, curr) pairs equals the operator call byte for byte, in any order of the ids, and leaves counts,
    stamps, sequence numbers, the ring and hnet_sessions_last_timing as they were"""
    key, views, _ = O.yawed(11)
    _, _, _, other = S.cases(11)
    a, b = np.stack([key] * 4), np.concatenate([views[:2], other[None], views[3:4]])
    hyps, fine, fo = O.yaw_table(fref, *F.TABLE_30), F.fine_yaw_table(fref, *F.TABLE_30, 5), F.fine_opts(fref)
    s = fleet()
    ids = [0, 1, 2, 3]
    s.push(ids, a, t=[1.0, 1.0, 1.0, 1.0])
    s.push(ids, b, t=[2.0, 2.0, 2.0, 2.0])
    s.infer([0, 2], np.zeros((2, 8)))
    ref, _ = F.ref_run(fref, a, b, S.search_opts(), hyps, fo, fine)
    before = [(s.seq(c), s.image_count(c), s.latest_time(c)) for c in ids]
    timing = s.last_timing()
    for order in ([0, 1, 2, 3], [3, 1], [2], [2, 3, 0]):
        out = s.photo_search_fine(order, hyps=hyps, fine=fine)
        assert out.tobytes() == ref[order].tobytes() == eng.op_photo_search_fine(a[order], b[order], hyps=hyps, fine=fine).tobytes()
    assert [(s.seq(c), s.image_count(c), s.latest_time(c)) for c in ids] == before and s.last_timing() == timing
    assert all(s.frame(c, 1).tobytes() == b[c].tobytes() and s.frame(c, 0).tobytes() == a[c].tobytes() for c in ids)
    assert set(ref["fine"]["flags"]) == {_capi.PSF_REFINED, _capi.PSF_SKIPPED}


def test_refusals_write_nothing(eng, fleet, fref):
    """the oriented call's refusals, and: null fine options, a null fine table, n_fine outside 1 .. 9, a radius outside 0 .. 4, a min_score outside
    [-1, 1] or NaN, an invalid fine entry: each returns its code and writes nothing"""
    L = _capi.lib()
    key, views, _ = O.yawed(1)
    a, b = np.stack([key] * 9), np.concatenate([views, views[:4]])
    out = np.full(9 * F.FREC.itemsize, 0xA5, np.uint8)
    sc = np.full(9 * 9 * 81, np.nan)
    keep, ok, fok = out.copy(), S.search_opts(), F.fine_opts(fref, n_fine=3)
    tab = O.table(fref, *O.TABLE5)
    fine = F.fine_rows(fref, *F.around(O.TABLE5, 3, 6.0))

    def bad_fine(field, k, v):
        t = fine.copy()
        t[field][4, 2][k] = v
        return t
    bad_fines = [bad_fine("a", 0, np.nan), bad_fine("a", 3, np.inf), bad_fine("b", 2, 2 * 65536 + 1), bad_fine("b", 0, -2 * 65536 - 1)]
    bad_fopts = [dict(n_fine=0), dict(n_fine=10), dict(radius=-1), dict(radius=5), dict(min_score=float("nan")), dict(min_score=1.5), dict(min_score=-1.5)]

    def op(i1, i2, n, o, t=tab, n_hyp=5, fo=fok, f=fine, outp=out.ctypes.data):
        return L.hnet_op_photo_search_fine(eng._h, i1.ctypes.data if i1 is not None else None, i2.ctypes.data if i2 is not None else None, n,
                                           C.addressof(o) if o is not None else None, t.ctypes.data if t is not None else None, n_hyp,
                                           C.addressof(fo) if fo is not None else None, f.ctypes.data if f is not None else None, outp, sc.ctypes.data)
    assert op(None, b, 1, ok) == INVALID and op(a, None, 1, ok) == INVALID and op(a, b, 1, None) == INVALID and op(a, b, 1, ok, outp=None) == INVALID
    assert op(a, b, 0, ok) == INVALID and op(a, b, 9, ok) == CAPACITY
    assert op(a, b, 1, ok, n_hyp=0) == INVALID and op(a, b, 1, ok, n_hyp=65) == INVALID and op(a, b, 1, ok, t=None) == INVALID
    assert op(a, b, 1, S.search_opts(radius_x=31)) == INVALID and op(a, b, 1, S.search_opts(min_overlap=15)) == INVALID
    assert op(a, b, 1, ok, fo=None) == INVALID and op(a, b, 1, ok, f=None) == INVALID
    for f in bad_fines:
        assert op(a, b, 1, ok, f=f) == INVALID
    for bad in bad_fopts:
        assert op(a, b, 1, ok, fo=F.fine_opts(fref, **{**dict(n_fine=3), **bad})) == INVALID, bad
    s = fleet()
    s.push([0, 1], a[:2])
    s.push([0], b[:1])

    def ses(ids, o, t=tab, n_hyp=5, fo=fok, f=fine, outp=out.ctypes.data):
        ids = np.asarray(ids, np.int32)
        return L.hnet_sessions_photo_search_fine(s._s, len(ids), ids.ctypes.data, C.addressof(o) if o is not None else None, t.ctypes.data if t is not None else None,
                                                 n_hyp, C.addressof(fo) if fo is not None else None, f.ctypes.data if f is not None else None, outp)
    assert ses([0, 0], ok) == INVALID and ses([4], ok) == INVALID and ses([], ok) == INVALID and ses([0], None) == INVALID and ses([0], ok, outp=None) == INVALID
    assert ses([0, 1], ok) == NOT_READY and ses([2], ok) == NOT_READY and ses([0, 1, 2, 3, 0, 1, 2, 3, 0], ok) == CAPACITY
    assert ses([0], ok, n_hyp=0) == INVALID and ses([0], ok, t=None) == INVALID and ses([0], ok, fo=None) == INVALID and ses([0], ok, f=None) == INVALID
    for f in bad_fines:
        assert ses([0], ok, f=f) == INVALID
    for bad in bad_fopts:
        assert ses([0], ok, fo=F.fine_opts(fref, **{**dict(n_fine=3), **bad})) == INVALID, bad
    assert out.tobytes() == keep.tobytes() and np.isnan(sc).all()
    assert s.photo_search_fine([0], hyps=tab, fine=fine, fine_opts=F.fine_kw(fok)).tobytes() == eng.op_photo_search_fine(a[:1], b[:1], hyps=tab, fine=fine,
                                                                                                                         fine_opts=F.fine_kw(fok)).tobytes()
