"""The coarse search under a table of orientation hypotheses on the device (include/hnet.h hnet_op_photo_search_oriented,
hnet_sessions_photo_search_oriented; csrc/kernels_photo_search_oriented.hip) against the host reference
tests/cpp/photo_search_oriented_ref.cpp, byte for byte: the warp and the sums are integers and the score is three correctly rounded double operations, so
there is no tolerance anywhere in this file.  Sessions objects of 4 cameras on a context of max_batch 8."""
import ctypes as C

import numpy as np
import pytest

import photo_search_oriented_util as O
import photo_search_util as S
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, CAPACITY = 1, 4, 5
N_CAM = 4


@pytest.fixture(scope="module")
def oref(tmp_path_factory):
    return O.build_ref(tmp_path_factory.mktemp("photo_search_oriented_ref_gpu"))


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
    keys = ["hyp", "hyp2", "n_scored", "score2"]
    assert dev.tobytes() == ref.tobytes(), (dev[keys], ref[keys], dev["base"][["dx", "dy", "flags", "score", "second"]], ref["base"][["dx", "dy", "flags", "score", "second"]])
    assert sc.shape == rsc.shape and sc.tobytes() == rsc.tobytes()


def test_tables_are_the_header_s(oref):
    """hnet_photo_search_make_hyp / _yaw_table give the host reference's entries byte for byte; the default table is 60 x 6 degrees from -180"""
    assert _capi.photo_search_yaw_table().tobytes() == O.yaw_table(oref).tobytes() == _capi.photo_search_table(None).tobytes()
    assert _capi.photo_search_yaw_table(-36.0, 6.0, 13).tobytes() == O.yaw_table(oref, -36.0, 6.0, 13).tobytes()
    assert _capi.photo_search_hyp(np.deg2rad(30.0), 0.8).tobytes() == O.hyp(oref, 30.0, 0.8).tobytes()
    out = np.zeros(60, O.HYP)
    assert _capi.lib().hnet_photo_search_default_yaw_table(out.ctypes.data) == 60 and out.tobytes() == O.yaw_table(oref).tobytes()
    with pytest.raises(ValueError):
        _capi.photo_search_hyp(0.0, 2.5)
    with pytest.raises(ValueError):
        _capi.photo_search_yaw_table(0.0, 1.0, 65)


@pytest.mark.parametrize("seed", S.SEEDS)
def test_identity_table(eng, oref, seed):
    """n = 1 with the identity table: the record and the score table equal the host reference, and the first 96 bytes hnet_op_photo_search's"""
    key, views, _, _ = S.cases(seed)
    a, b = key[None], views[seed % 4][None]
    ident, o = O.table(oref, *O.IDENTITY), S.search_opts()
    ref, rsc = O.ref_run(oref, a, b, o, ident)
    dev, sc = eng.op_photo_search_oriented(a, b, hyps=ident, want_scores=True)
    _same(dev, sc, ref, rsc)
    plain, psc = eng.op_photo_search(a, b, want_scores=True)
    assert dev[0].tobytes()[:96] == plain[0].tobytes() and sc[:, 0].tobytes() == psc.tobytes() and dev["base"]["flags"][0] == _capi.PS_FOUND


@pytest.mark.parametrize("seed", S.SEEDS)
def test_five_entries_in_two_slot_orders(eng, oref, seed):
    """n = 3 in two slot orders with a 5-entry table that holds a quarter turn and scaled entries: every record and the whole score table equal the host
    reference byte for byte; a pair's bytes are the same in any slot"""
    key, views, _ = O.yawed(seed)
    _, _, _, other = S.cases(seed)
    a, b = np.stack([key] * 4), np.concatenate([views[:3], other[None]])
    tab, o = O.table(oref, *O.TABLE5), S.search_opts()
    ref, rsc = O.ref_run(oref, a, b, o, tab)
    for order in ([0, 3, 2], [2, 1, 0]):
        dev, sc = eng.op_photo_search_oriented(a[order], b[order], hyps=tab, want_scores=True)
        _same(dev, sc, ref[order], rsc[order])
        assert eng.op_photo_search_oriented(a[order], b[order], hyps=tab).tobytes() == ref[order].tobytes()      # (without the tables: the same records)


def test_64_entries_and_the_default_table(eng, oref):
    """n = 1 with 64 entries, and the yawed rows of a seed under the default table (hyps = None): byte for byte the host reference, FOUND where 7r's
    search on the device is not"""
    key, views, poses = O.yawed(5)
    tab, o = O.yaw_table(oref, -180.0, 5.625, 64), S.search_opts()
    ref, rsc = O.ref_run(oref, key[None], views[1:2], o, tab)
    dev, sc = eng.op_photo_search_oriented(key[None], views[1:2], hyps=tab, want_scores=True)
    _same(dev, sc, ref, rsc)
    assert dev["n_scored"][0] == 64 and dev["base"]["flags"][0] == _capi.PS_FOUND
    keys = np.stack([key] * len(views))
    ref, rsc = O.ref_run(oref, keys, views, o, O.yaw_table(oref))
    dev, sc = eng.op_photo_search_oriented(keys, views, want_scores=True)
    _same(dev, sc, ref, rsc)
    plain = eng.op_photo_search(keys, views)
    assert (dev["base"]["flags"] == _capi.PS_FOUND).all() and (plain["flags"] != _capi.PS_FOUND).all()
    assert all(S.worst_px(dev["base"]["start_px"][i], poses[i]) <= O.BASIN_PX for i in range(len(views)))


def test_full_batch_radii_and_min_overlap(eng, oref):
    """n = max_batch = 8 at radii 26 x 7 and min_overlap 16: the tables are NaN outside the radii, byte for byte the reference"""
    k2, v2, _ = O.yawed(2)
    k11, v11, _ = O.yawed(11)
    a, b = np.stack([k2] * 5 + [k11] * 3), np.concatenate([v2, v11[:3]])
    tab = O.table(oref, *O.TABLE5)
    o = S.search_opts(radius_x=26, radius_y=7, min_overlap=16, min_score=0.5, min_margin=0.05)
    ref, rsc = O.ref_run(oref, a, b, o, tab)
    dev, sc = eng.op_photo_search_oriented(a, b, hyps=tab, want_scores=True, **S.search_kw(o))
    _same(dev, sc, ref, rsc)
    assert np.isnan(sc[:, :, :, :4]).all() and np.isnan(sc[:, :, :13, :]).all() and not np.isnan(sc[:, 0, 13, 4]).any()


def test_hand_built_cases(eng, oref):
    """the hand-built cases as frames of constant 8 x 8 blocks, each alone with its own options and table, and together in one call of 5 under one table
    that holds all their entries: byte for byte the host reference"""
    h = O.hand_built()
    for name, (ta, tb, o, entries) in h.items():
        a, b, tab = S.expand(ta)[None], S.expand(tb)[None], O.table(oref, *entries)
        ref, rsc = O.ref_run(oref, a, b, o, tab)
        want, _, _ = O.ref_search(oref, ta, tb, o, tab)
        assert ref.tobytes() == want.tobytes(), name
        dev, sc = eng.op_photo_search_oriented(a, b, hyps=tab, want_scores=True, **S.search_kw(o))
        _same(dev, sc, ref, rsc)
    names = sorted(h)
    a, b = np.stack([S.expand(h[n][0]) for n in names]), np.stack([S.expand(h[n][1]) for n in names])
    tab, o = O.table(oref, (0.0, 0.5), (10.0, 1.0), (0.0, 1.0), (0.0, 1.0), (90.0, 1.0)), S.search_opts(min_overlap=32)
    ref, rsc = O.ref_run(oref, a, b, o, tab)
    dev, sc = eng.op_photo_search_oriented(a, b, hyps=tab, want_scores=True, **S.search_kw(o))
    _same(dev, sc, ref, rsc)
    got = dict(zip(names, dev))
    assert got["constant-template"]["base"]["flags"] == _capi.PS_NO_TEXTURE and got["constant-template"]["hyp"] == -1
    assert (got["same-matrix-twice"]["hyp"], got["same-matrix-twice"]["hyp2"]) == (2, 3)
    e = got["edge-peak-under-90"]
    assert (e["hyp"], e["base"]["dx"], e["base"]["dy"], e["base"]["n_overlap"]) == (4, 30, 20, 32)


def test_sessions_call(eng, fleet, oref):
    """hnet_sessions_photo_search_oriented on the (prev, curr) pairs equals the operator call byte for byte, in any order of the ids, and leaves counts,
    stamps, sequence numbers, the ring and hnet_sessions_last_timing as they were"""
    key, views, _ = O.yawed(11)
    _, _, _, other = S.cases(11)
    a, b = np.stack([key] * 4), np.concatenate([views[:2], other[None], views[3:4]])
    tab = O.yaw_table(oref, -36.0, 6.0, 13)
    s = fleet()
    ids = [0, 1, 2, 3]
    s.push(ids, a, t=[1.0, 1.0, 1.0, 1.0])
    s.push(ids, b, t=[2.0, 2.0, 2.0, 2.0])
    s.infer([0, 2], np.zeros((2, 8)))
    ref, _ = O.ref_run(oref, a, b, S.search_opts(), tab)
    before = [(s.seq(c), s.image_count(c), s.latest_time(c)) for c in ids]
    timing = s.last_timing()
    for order in ([0, 1, 2, 3], [3, 1], [2], [2, 3, 0]):
        out = s.photo_search_oriented(order, hyps=tab)
        assert out.tobytes() == ref[order].tobytes() == eng.op_photo_search_oriented(a[order], b[order], hyps=tab).tobytes()
    assert [(s.seq(c), s.image_count(c), s.latest_time(c)) for c in ids] == before and s.last_timing() == timing
    assert all(s.frame(c, 1).tobytes() == b[c].tobytes() and s.frame(c, 0).tobytes() == a[c].tobytes() for c in ids)
    assert s.photo_search_oriented([1]).tobytes() == eng.op_photo_search_oriented(a[1:2], b[1:2]).tobytes()           # the default table


def test_refusals_write_nothing(eng, fleet, oref):
    """null arguments, n = 0, n > max_batch, an option out of range, a table of 0 or 65 entries, a null table, a non-finite entry, an entry past the
    scale's range, a repeated id, a session without a pair: each returns its code and writes nothing"""
    L = _capi.lib()
    key, views, _ = O.yawed(1)
    a, b = np.stack([key] * 9), np.concatenate([views, views[:4]])
    out = np.full(9 * O.OREC.itemsize, 0xA5, np.uint8)
    sc = np.full(9 * 3 * S.NSX * S.NSY, np.nan)
    keep, ok = out.copy(), S.search_opts()
    tab = np.zeros(65, O.HYP)
    tab[:] = O.table(oref, *O.IDENTITY)[0]
    tab[:5] = O.table(oref, *O.TABLE5)

    def bad_table(field, k, v):
        t = tab[:3].copy()
        t[field][1][k] = v
        return t
    bad_tables = [bad_table("a", 0, np.nan), bad_table("a", 3, np.inf), bad_table("b", 2, 2 * 65536 + 1), bad_table("b", 0, -2 * 65536 - 1)]

    def op(i1, i2, n, o, t=tab, n_hyp=3, outp=out.ctypes.data):
        return L.hnet_op_photo_search_oriented(eng._h, i1.ctypes.data if i1 is not None else None, i2.ctypes.data if i2 is not None else None, n,
                                               C.addressof(o) if o is not None else None, t.ctypes.data if t is not None else None, n_hyp, outp, sc.ctypes.data)
    assert op(None, b, 1, ok) == INVALID and op(a, None, 1, ok) == INVALID and op(a, b, 1, None) == INVALID and op(a, b, 1, ok, outp=None) == INVALID
    assert op(a, b, 0, ok) == INVALID and op(a, b, 9, ok) == CAPACITY
    assert op(a, b, 1, ok, n_hyp=0) == INVALID and op(a, b, 1, ok, n_hyp=65) == INVALID and op(a, b, 1, ok, n_hyp=-1) == INVALID and op(a, b, 1, ok, t=None) == INVALID
    for t in bad_tables:
        assert op(a, b, 1, ok, t=t) == INVALID
    bads = (dict(radius_x=31), dict(radius_y=-1), dict(min_overlap=15), dict(min_overlap=1121), dict(min_score=float("nan")), dict(min_margin=2.01))
    for bad in bads:
        assert op(a, b, 1, S.search_opts(**bad)) == INVALID, bad
    s = fleet()
    s.push([0, 1], a[:2])
    s.push([0], b[:1])

    def ses(ids, o, t=tab, n_hyp=3, outp=out.ctypes.data):
        ids = np.asarray(ids, np.int32)
        return L.hnet_sessions_photo_search_oriented(s._s, len(ids), ids.ctypes.data, C.addressof(o) if o is not None else None,
                                                     t.ctypes.data if t is not None else None, n_hyp, outp)
    assert ses([0, 0], ok) == INVALID and ses([4], ok) == INVALID and ses([], ok) == INVALID and ses([0], None) == INVALID and ses([0], ok, outp=None) == INVALID
    assert ses([0, 1], ok) == NOT_READY and ses([2], ok) == NOT_READY and ses([0, 1, 2, 3, 0, 1, 2, 3, 0], ok) == CAPACITY
    assert ses([0], ok, n_hyp=0) == INVALID and ses([0], ok, n_hyp=65) == INVALID and ses([0], ok, t=None) == INVALID
    for t in bad_tables:
        assert ses([0], ok, t=t) == INVALID
    for bad in bads:
        assert ses([0], S.search_opts(**bad)) == INVALID, bad
    assert out.tobytes() == keep.tobytes() and np.isnan(sc).all()
    assert s.photo_search_oriented([0], hyps=tab[:3]).tobytes() == eng.op_photo_search_oriented(a[:1], b[:1], hyps=tab[:3]).tobytes()
