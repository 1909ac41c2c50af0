"""The three search stages at the edges of their shift domain on the device (include/hnet.h hnet_op_photo_search, hnet_op_photo_search_oriented,
hnet_op_photo_search_fine, hnet_sessions_keyframe_relocalise_fine; csrc/kernels_photo_search.hip, kernels_photo_search_oriented.hip,
kernels_photo_search_fine.hip): the cases of tests/photo_search_hostile.py, whose conditions tests/test_photo_search_hostile_cpu.py checks
on the host reference.  Every device call, with want_scores, equals the host reference byte for byte, records and whole score tables: the sums are
integers and the score is three correctly rounded double operations, so the file has no tolerance and no comparison leaves a shift out.  One table goes
to both sides.  Calls of up to 8 pairs on a context of max_batch 8; sessions objects of 4 cameras."""
import numpy as np
import pytest

import photo_search_fine_util as F
import photo_search_hostile as H
import photo_search_oriented_util as O
import photo_search_util as S
import test_gpu_keyframe_reloc_fine as RF
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

N_CAM = 4


@pytest.fixture(scope="module")
def fref(tmp_path_factory):
    return F.build_ref(tmp_path_factory.mktemp("photo_search_hostile_ref_gpu"))


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

    def make(capacity):
        s = HnetSessions(eng, N_CAM)
        s.enable_keyframes()
        if capacity:
            s.enable_keyframe_map(capacity)
        made.append(s)
        return s
    yield make
    for s in made:
        s.close()


def _call(eng, lib, cases, call):
    """one device call on the pairs of `cases`, which share options and tables, and the host reference: equal byte for byte -> (records, score tables)"""
    c = cases[0]
    assert 1 <= len(cases) <= 8 and len(H.batches(dict(enumerate(cases)))) == 1
    a, b = (np.stack(x) for x in zip(*(H.frames(x, call) for x in cases)))
    hyps, fo, fine = H.tables(lib, c)
    kw = S.search_kw(c.o)
    if call == "coarse":
        ref, rsc = S.ref_run(lib, a, b, c.o)
        dev, sc = eng.op_photo_search(a, b, want_scores=True, **kw)
        keys = ["dx", "dy", "flags", "score", "second"]
        assert dev.tobytes() == ref.tobytes(), (dev[keys], ref[keys])
    elif call == "oriented":
        ref, rsc = O.ref_run(lib, a, b, c.o, hyps)
        dev, sc = eng.op_photo_search_oriented(a, b, hyps=hyps, want_scores=True, **kw)
        keys = ["dx", "dy", "flags", "score", "second"]
        assert dev.tobytes() == ref.tobytes(), (dev["hyp"], ref["hyp"], dev["base"][keys], ref["base"][keys])
    else:
        ref, rsc = F.ref_run(lib, a, b, c.o, hyps, fo, fine)
        dev, sc = eng.op_photo_search_fine(a, b, hyps=hyps, fine=fine, fine_opts=F.fine_kw(fo), want_scores=True, **kw)
        keys = ["flags", "j", "ex", "ey", "sx", "sy", "score", "n_overlap", "sa", "sb", "sab", "saa", "sbb"]
        assert dev.tobytes() == ref.tobytes(), (dev["fine"][keys], ref["fine"][keys], dev["coarse"][["hyp", "n_scored"]], ref["coarse"][["hyp", "n_scored"]])
        assert dev["coarse"].tobytes() == eng.op_photo_search_oriented(a, b, hyps=hyps, **kw).tobytes()
    assert sc.shape == rsc.shape and sc.tobytes() == rsc.tobytes(), np.argwhere(sc.view(np.uint64) != rsc.view(np.uint64))[:8]
    return dev, sc


def _group(eng, lib, cases, names):
    return {call: _call(eng, lib, [cases[n] for n in names], call) for call in cases[names[0]].calls}


@pytest.mark.parametrize("names", H.batches(H.corners()), ids=lambda n: f"{n[0]}+{len(n) - 1}")
def test_corners_and_edges(eng, fref, names):
    """group 1: the nine sign combinations of the coarse corners and edges at the even and at an odd level-2 offset, half of them under the half turn, in
    the coarse, the oriented and the fine call: the fine shifts reach all four corners (+-64, +-44) of the level-2 domain"""
    out = _group(eng, fref, H.corners(), names)
    for i, n in enumerate(names):
        w, p = H.corners()[n].want, out["fine"][0][i]["fine"]
        assert (p["flags"], p["sx"], p["sy"], p["j"], out["oriented"][0][i]["hyp"]) == (_capi.PSF_REFINED, w["fine"][0], w["fine"][1], w["j"], w["hyp"])
        assert out["coarse"][0][i]["flags"] == _capi.PS_FOUND


@pytest.mark.parametrize("name", H.THRESHOLDS)
def test_overlap_threshold_at_equality(eng, fref, name):
    """group 2: min_overlap at the chosen shift's n, read from the host reference, and one above: scored, then NaN"""
    at, above, call, idx, n = H.threshold_runs(fref, name)
    _, sc_at = _call(eng, fref, [at], call)
    _, sc_above = _call(eng, fref, [above], call)
    assert not np.isnan(sc_at[0][idx]) and np.isnan(sc_above[0][idx])


@pytest.mark.parametrize("names", H.batches(H.number_range()), ids=lambda n: f"{n[0]}+{len(n) - 1}")
def test_number_range(eng, fref, names):
    """group 3: bytes of {254, 255}, {0, 1} and {0, 255}: sums up to 4 480 x 255^2 and variances that are small but positive; a constant 255 template;
    the bright pair under a ragged 45 degree mask"""
    out = _group(eng, fref, H.number_range(), names)
    for i, n in enumerate(names):
        w, p = H.number_range()[n].want, out["fine"][0][i]["fine"]
        assert p["flags"] == (_capi.PSF_SKIPPED if w.get("skipped") else _capi.PSF_LOW_SCORE if w.get("masked") else _capi.PSF_REFINED)
        if n == "bright(0,0)":
            assert p["sbb"] > 1 << 28


@pytest.mark.parametrize("names", H.batches(H.single_pixels()), ids=lambda n: f"{n[0]}+{len(n) - 1}")
def test_zero_variance_inside_a_scored_table(eng, fref, names):
    """group 4: one pixel in a constant template: a byte mask that is off by one column turns a NaN into a score or a score into a NaN"""
    out = _group(eng, fref, H.single_pixels(), names)
    for call in ("coarse", "fine"):
        assert all(0 < np.isnan(sc).sum() < sc.size or n in ("pixel(4,28)", "pixel(75,28)") for n, sc in zip(names, out[call][1]))


def test_neighbours_in_one_call(eng, fref):
    """group 5: SKIPPED, NOTHING_SCORED, LOW_SCORE and corner REFINED pairs interleaved in one call of 8: each record and table equals the one the pair
    gets alone; a SKIPPED pair's table is quiet NaN in the header's bits"""
    cases = list(H.neighbours())
    dev, sc = _call(eng, fref, cases, "fine")
    assert [int(f) for f in dev["fine"]["flags"]] == [c.want["flags"] for c in cases]
    for i, (c, kind) in enumerate(zip(cases, H.NEIGHBOUR_KINDS)):
        alone, asc = _call(eng, fref, [c], "fine")
        assert alone[0].tobytes() == dev[i].tobytes() and asc[0].tobytes() == sc[i].tobytes(), (i, kind)
        if kind == "skipped":
            assert np.array_equal(sc[i].view(np.uint64), np.full(sc[i].shape, H.QNAN64, np.uint64))
            assert np.array_equal(dev[i]["fine"]["start_px"].view(np.uint32), F.NAN32)


class _Tabs:
    """the tables of a case in the form test_gpu_keyframe_reloc_fine.Cam takes"""

    def __init__(self, lib, c):
        self.hyps, self.fo, self.fine = H.tables(lib, c)
        self.kw = dict(hyps=self.hyps, fine=self.fine, fine_opts=F.fine_kw(self.fo))


@pytest.mark.parametrize("capacity", [0, _capi.KEYFRAME_MAP_MAX_CAPACITY])
@pytest.mark.parametrize("name", ["even(30,20)", "odd(-30,-20)"])
def test_one_relocalisation(eng, fleet, fref, name, capacity):
    """group 6: hnet_sessions_keyframe_relocalise_fine with the template as the keyframe and the image as the pushed frame, without a map and with the
    largest: the record equals the host headers on the device's alignment record, and its coarse and fine parts the operator calls', byte for byte"""
    c = H.corners()[name]
    a, b = H.frames(c, "fine")
    tabs = _Tabs(fref, c)
    cam = RF.Cam(fleet(capacity), 2, fref, capacity, tabs)
    cam.track(a, None, RF.KIDNAP)
    cam.track(b, None, RF.KIDNAP)
    o = S.reloc_opts(search=c.o)
    rl = cam.relocalise(b, o)
    RF._pinned(eng, rl, a, b, o, tabs)
    p = rl["fine"]
    assert (p["flags"], p["sx"], p["sy"], p["j"], rl["base"]["search"]["hyp"]) == (_capi.PSF_REFINED, c.want["fine"][0], c.want["fine"][1], c.want["j"], c.want["hyp"])
