"""The coarse search over integer translations on the device (include/hnet.h hnet_op_photo_search, hnet_sessions_photo_search;
csrc/kernels_photo_search.hip) against the host reference tests/cpp/photo_search_ref.cpp, byte for byte: the quantity is integer sums and three
correctly rounded double operations, so there is no tolerance anywhere in this file.  Sessions objects of 4 cameras on a context of max_batch 8."""
import ctypes as C

import numpy as np
import pytest

import photo_search_util as S
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, CAPACITY = 1, 4, 5
N_CAM = 4


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return S.build_ref(tmp_path_factory.mktemp("photo_search_ref_gpu"))


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


def _pairs(seed):
    """the five pairs of a seed: the keyframe against its four views and against the unrelated frame"""
    key, views, _, other = S.cases(seed)
    return np.stack([key] * 5), np.concatenate([views, other[None]])


def _same(dev, sc, ref, rsc):
    assert dev.tobytes() == ref.tobytes(), (dev[["dx", "dy", "flags", "score", "second"]], ref[["dx", "dy", "flags", "score", "second"]])
    assert sc.tobytes() == rsc.tobytes()


@pytest.mark.parametrize("seed", S.SEEDS)
def test_views_equal_the_reference(eng, sref, seed):
    """n = 1 and n = 3 in two slot orders on the views and the unrelated frame: every record and the whole score table equal the host reference byte for
    byte; a pair's bytes are the same alone, in slot 0, in the last slot and beside a NO_TEXTURE pair"""
    a, b = _pairs(seed)
    o = S.search_opts()
    ref, rsc = S.ref_run(sref, a, b, o)
    assert (ref["flags"][:4] == _capi.PS_FOUND).all() and ref["flags"][4] == _capi.PS_LOW_SCORE
    for i in range(5):
        dev, sc = eng.op_photo_search(a[i:i + 1], b[i:i + 1], want_scores=True)
        _same(dev, sc, ref[i:i + 1], rsc[i:i + 1])
    for order in ([0, 4, 2], [2, 0, 4], [3, 1, 0], [1, 3, 4]):
        dev, sc = eng.op_photo_search(a[order], b[order], want_scores=True)
        _same(dev, sc, ref[order], rsc[order])
        assert eng.op_photo_search(a[order], b[order]).tobytes() == ref[order].tobytes()          # (without the table: the same records)
    flat = np.full((1, 224, 320), 200, np.uint8)
    mix = eng.op_photo_search(np.concatenate([flat, a[:1]]), np.concatenate([b[:1], b[:1]]))            # beside a NO_TEXTURE pair
    assert mix[0]["flags"] == _capi.PS_NO_TEXTURE and mix[1].tobytes() == ref[0].tobytes()


def test_hostile_thumbnails_equal_the_reference(eng, sref):
    """the hand-built thumbnails as frames of constant 8 x 8 blocks, each with its own options, alone and - those that share the default options - in one
    call of 5 beside the NO_TEXTURE pairs: byte for byte the host reference"""
    h = S.hostile()
    for name, (ta, tb, o, _) in h.items():
        a, b = S.expand(ta)[None], S.expand(tb)[None]
        ref, rsc = S.ref_run(sref, a, b, o)
        want, _ = S.ref_search(sref, ta, tb, o)
        assert ref.tobytes() == want.tobytes(), name
        dev, sc = eng.op_photo_search(a, b, want_scores=True, **S.search_kw(o))
        _same(dev, sc, ref, rsc)
    names = [n for n in h if bytes(h[n][2]) == bytes(S.search_opts())]
    assert "constant-image" in names and "constant-template" in names and len(names) >= 5
    a, b = np.stack([S.expand(h[n][0]) for n in names]), np.stack([S.expand(h[n][1]) for n in names])
    ref, rsc = S.ref_run(sref, a, b, S.search_opts())
    dev, sc = eng.op_photo_search(a, b, want_scores=True)
    _same(dev, sc, ref, rsc)
    flags = dict(zip(names, dev["flags"]))
    assert flags["constant-image"] == flags["constant-template"] == _capi.PS_NO_TEXTURE and flags["checker"] == _capi.PS_AMBIGUOUS


def test_full_batch_and_radii(eng, sref):
    """n = max_batch = 8 with radii below the range and a low min_overlap: the table is NaN outside the radii, byte for byte the reference"""
    a1, b1 = _pairs(2)
    a2, b2 = _pairs(5)
    a, b = np.concatenate([a1, a2[:3]]), np.concatenate([b1, b2[:3]])
    o = S.search_opts(radius_x=26, radius_y=7, min_overlap=16, min_score=0.5, min_margin=0.05)
    ref, rsc = S.ref_run(sref, a, b, o)
    dev, sc = eng.op_photo_search(a, b, want_scores=True, **S.search_kw(o))
    _same(dev, sc, ref, rsc)
    assert np.isnan(sc[:, :, :4]).all() and np.isnan(sc[:, :13, :]).all() and not np.isnan(sc[:, 13, 4]).any()


def test_sessions_call(eng, fleet, sref):
    """hnet_sessions_photo_search on the (prev, curr) pairs equals the operator call byte for byte, in any order of the ids, and leaves counts, stamps,
    sequence numbers and hnet_sessions_last_timing as they were"""
    a, b = _pairs(11)
    s = fleet()
    ids = [0, 1, 2, 3]
    s.push(ids, a[:4], t=[1.0, 1.0, 1.0, 1.0])
    s.push(ids, b[[0, 1, 4, 3]], t=[2.0, 2.0, 2.0, 2.0])
    s.infer([0, 2], np.zeros((2, 8)))
    ref, _ = S.ref_run(sref, a[:4], b[[0, 1, 4, 3]], S.search_opts())
    before = [(s.seq(c), s.image_count(c), s.latest_time(c)) for c in ids]
    timing = s.last_timing()
    for order in ([0, 1, 2, 3], [3, 1], [2], [2, 3, 0]):
        out = s.photo_search(order)
        assert out.tobytes() == ref[order].tobytes() == eng.op_photo_search(a[order], b[[0, 1, 4, 3]][order]).tobytes()
    assert [(s.seq(c), s.image_count(c), s.latest_time(c)) for c in ids] == before and s.last_timing() == timing
    assert s.frame(2, 1).tobytes() == b[4].tobytes() and s.frame(2, 0).tobytes() == a[2].tobytes()


def test_refusals_write_nothing(eng, fleet):
    """null arguments, n = 0, n > max_batch, every option out of range, a repeated id, a session without a pair: each returns its code and writes nothing"""
    L = _capi.lib()
    a, b = _pairs(1)
    out = np.full(9 * S.SEARCH.itemsize, 0xA5, np.uint8)
    sc = np.full(9 * S.NSX * S.NSY, np.nan)
    keep, ok = out.copy(), S.search_opts()
    big_a, big_b = np.concatenate([a, a[:4]]), np.concatenate([b, b[:4]])

    def op(i1, i2, n, o, outp=out.ctypes.data):
        return L.hnet_op_photo_search(eng._h, i1.ctypes.data if i1 is not None else None, i2.ctypes.data if i2 is not None else None, n,
                                      C.addressof(o) if o is not None else None, outp, sc.ctypes.data)
    assert op(None, b, 1, ok) == INVALID and op(a, None, 1, ok) == INVALID and op(a, b, 1, None) == INVALID and op(a, b, 1, ok, outp=None) == INVALID
    assert op(a, b, 0, ok) == INVALID and op(big_a, big_b, 9, ok) == CAPACITY
    assert L.hnet_op_photo_search(None, a.ctypes.data, b.ctypes.data, 1, C.addressof(ok), out.ctypes.data, None) == INVALID
    bads = (dict(radius_x=-1), dict(radius_x=31), dict(radius_y=-1), dict(radius_y=21), dict(min_overlap=15), dict(min_overlap=1121), dict(min_score=-1.01),
            dict(min_score=1.01), dict(min_score=float("nan")), dict(min_margin=-0.01), dict(min_margin=2.01), dict(min_margin=float("nan")))
    for bad in bads:
        assert op(a, b, 1, S.search_opts(**bad)) == INVALID, bad
    s = fleet()
    s.push([0, 1], a[:2])
    s.push([0], b[:1])

    def ses(ids, o, outp=out.ctypes.data):
        ids = np.asarray(ids, np.int32)
        return L.hnet_sessions_photo_search(s._s, len(ids), ids.ctypes.data, C.addressof(o) if o is not None else None, outp)
    assert ses([0, 0], ok) == INVALID and ses([4], ok) == INVALID and ses([], ok) == INVALID and ses([0], None) == INVALID and ses([0], ok, outp=None) == INVALID
    assert ses([0, 1], ok) == NOT_READY and ses([2], ok) == NOT_READY and ses([0, 1, 2, 3, 0, 1, 2, 3, 0], ok) == CAPACITY
    for bad in bads:
        assert ses([0], S.search_opts(**bad)) == INVALID, bad
    assert L.hnet_sessions_photo_search(None, 1, None, None, None) == INVALID
    assert out.tobytes() == keep.tobytes() and np.isnan(sc).all()
    assert s.photo_search([0]).tobytes() == eng.op_photo_search(a[:1], b[:1]).tobytes()
