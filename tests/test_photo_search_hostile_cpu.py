"""The three search stages at the edges of their shift domain (include/hnet_photo_search.h, hnet_photo_search_oriented.h, hnet_photo_search_fine.h;
DESIGN 7x) on the CPU: for every case of tests/photo_search_hostile.py the host references - the functions the device compiles - equal the numpy
restatements (photo_search_util.np_search, photo_search_oriented_util.np_search, photo_search_fine_util.np_refine) byte for byte, records and whole score
tables, and the case meets its stated condition on the reference alone.  tests/test_gpu_photo_search_hostile.py then holds the device to the same
reference.  The sums are integers and the score is three correctly rounded double operations: no tolerance appears in this file."""
import numpy as np
import pytest

import photo_search_fine_util as F
import photo_search_hostile as H
import photo_search_oriented_util as O
import photo_search_util as S
from cuahn_vio_amd import _capi


@pytest.fixture(scope="module")
def fref(tmp_path_factory):
    return F.build_ref(tmp_path_factory.mktemp("photo_search_hostile_ref"))


def _same(a, b, dtype):
    """two records byte for byte, with a message that names the field"""
    for f in dtype.names:
        assert np.atleast_1d(a[f]).tobytes() == np.atleast_1d(b[f]).tobytes(), (f, a[f], b[f])
    assert a.tobytes() == b.tobytes()


def _bits(scores, table):
    assert scores.shape == table.shape and np.array_equal(scores.view(np.uint64), table.view(np.uint64))


def _reference(lib, c):
    """every call of the case on the host reference, each equal to the numpy restatement byte for byte -> call: (record, score table)"""
    hyps, fo, fine = H.tables(lib, c)
    out, b3 = {}, H.down2(c.b)
    if "coarse" in c.calls:
        a, b = H.frames(c, "coarse")
        rec, sc = S.ref_run(lib, a[None], b[None], c.o)
        want, table = S.np_search(H.down2(c.a), b3, c.o)
        _bits(sc[0], table)
        _same(rec[0], want[0], S.SEARCH)
        out["coarse"] = rec[0], sc[0]
    t2 = H.template(c, "fine")
    a, b = H.frames(c, "fine")
    orec, osc = O.ref_run(lib, a[None], b[None], c.o, hyps)
    if "oriented" in c.calls:
        want, table, _ = O.np_search(H.down2(t2), b3, c.o, hyps)
        _bits(osc[0], table)
        _same(orec[0], want[0], O.OREC)
        out["oriented"] = orec[0], osc[0]
    if "fine" in c.calls:
        rec, sc = F.ref_run(lib, a[None], b[None], c.o, hyps, fo, fine)
        assert rec[0]["coarse"].tobytes() == orec[0].tobytes()
        want, table = F.np_refine(t2, c.b, orec[0], c.o.min_overlap, fo, fine)
        _bits(sc[0], table)
        _same(rec[0]["fine"], want[0], F.PART)
        out["fine"] = rec[0], sc[0]
    return out


def _meets(c, out):
    """the case's `want` on the reference's records"""
    w = c.want
    bases = [out["coarse"][0]] if "coarse" in out else []
    for call in ("oriented", "fine"):
        if call in out:
            r = out[call][0] if call == "oriented" else out[call][0]["coarse"]
            bases.append(r["base"])
            if "hyp" in w:
                assert r["hyp"] == w["hyp"], (call, r["hyp"])
    if "coarse" in w:
        for r in bases:
            assert r["flags"] == _capi.PS_FOUND, r["flags"]
            if w["coarse"] is not None:
                assert (r["dx"], r["dy"]) == w["coarse"]
            else:                                  # a truth half a pixel between two level-3 shifts on each axis: one of the two nearest
                assert abs(2 * int(r["dx"]) - w["fine"][0]) <= 1 and abs(2 * int(r["dy"]) - w["fine"][1]) <= 1, (r["dx"], r["dy"])
    if "fine" in w and "fine" in out:
        p = out["fine"][0]["fine"]
        assert (p["flags"], p["sx"], p["sy"], p["j"]) == (_capi.PSF_REFINED, w["fine"][0], w["fine"][1], w["j"]) and p["score"] == 1.0
        assert np.array_equal(p["start_px"], F.np_start(p["a"], int(p["sx"]), int(p["sy"])))


# ---- group 1

@pytest.fixture(scope="module")
def corner_runs(fref):
    """name -> the reference's runs of a corner case, computed once"""
    done = {}

    def get(name):
        if name not in done:
            done[name] = _reference(fref, H.corners()[name])
        return done[name]
    return get


@pytest.mark.parametrize("name", sorted(H.corners()))
def test_corners_and_edges(corner_runs, name):
    """the coarse stage is FOUND at the intended shift (at the odd offsets: at one of the two nearest on each axis), under the intended entry; the fine
    stage is REFINED at the exact level-2 offset with score 1.0 from the lower of the two equal entries; all 81 fine shifts of the identity and of the
    half turn are scored"""
    c, out = H.corners()[name], corner_runs(name)
    _meets(c, out)
    rec, sc = out["fine"]
    p = rec["fine"]
    print(f"{name}: coarse entry {rec['coarse']['hyp']} ({rec['coarse']['base']['dx']}, {rec['coarse']['base']['dy']}) score {rec['coarse']['base']['score']:.4f}; "
          f"fine j {p['j']} ({p['sx']}, {p['sy']}) score {p['score']} n {p['n_overlap']}; NaN per entry {[int(np.isnan(sc[j]).sum()) for j in range(3)]}")
    twice = [j for j, e in enumerate(c.rows[c.want["hyp"]]) if e == c.entries[c.want["hyp"]]]
    assert len(twice) == 2 and twice[0] == c.want["j"]
    for j in twice:
        assert not np.isnan(sc[j]).any()
    assert np.array_equal(sc[twice[0]].view(np.uint64), sc[twice[1]].view(np.uint64))


def test_corners_cover_the_domain(corner_runs):
    """over the group every value of sx & 3 is scored for both signs of sx, and the four shifts (+-64, +-44) are each scored at least once"""
    seen, far = set(), set()
    for name in H.corners():
        rec, sc = corner_runs(name)["fine"]
        dx, dy = int(rec["coarse"]["base"]["dx"]), int(rec["coarse"]["base"]["dy"])
        for j, ey, ex in zip(*np.nonzero(~np.isnan(sc))):
            sx, sy = 2 * dx + int(ex) - 4, 2 * dy + int(ey) - 4
            seen.add((int(np.sign(sx)), sx & 3))
            if abs(sx) == H.MAX_SX and abs(sy) == H.MAX_SY:
                far.add((sx, sy))
    assert seen >= {(s, k) for s in (-1, 1) for k in range(4)}
    assert far == {(sx, sy) for sx in (-64, 64) for sy in (-44, 44)}


# ---- group 2

@pytest.mark.parametrize("name", H.THRESHOLDS)
def test_overlap_threshold_at_equality(fref, name):
    """with the threshold equal to the chosen shift's n the shift is scored, one above it is NaN; the thresholds come from the reference's record or sums"""
    at, above, call, idx, n = H.threshold_runs(fref, name)
    sc_at, sc_above = _reference(fref, at)[call], _reference(fref, above)[call]
    unit = 4 if call == "fine" else 1
    print(f"{name}: n {n} at index {idx}; thresholds {unit * at.o.min_overlap} and {unit * above.o.min_overlap}; NaN in the table {int(np.isnan(sc_at[1]).sum())} and "
          f"{int(np.isnan(sc_above[1]).sum())}")
    assert unit * at.o.min_overlap <= n < unit * above.o.min_overlap and above.o.min_overlap == at.o.min_overlap + 1
    assert not np.isnan(sc_at[1][idx]) and np.isnan(sc_above[1][idx])
    if name in ("coarse", "oriented"):
        assert at.o.min_overlap == n and (name == "oriented" or n == 80)      # (the oriented n is under a ragged mask: whatever the record says)
    if name == "fine":                             # the unmasked corner: 16 x 12 pixels = 4 * 48; one above, (64, 44) is the only shift that goes
        assert n == 192 and at.o.min_overlap == 48 and not np.isnan(sc_at[1]).any()
        assert int(np.isnan(sc_above[1]).sum()) == 1
    if name == "fine-45":                          # a ragged mask whose n is a multiple of 4: equality; the stage still runs on both sides of it
        assert n % 4 == 0 and 4 * at.o.min_overlap == n
        assert sc_at[0]["fine"]["flags"] == sc_above[0]["fine"]["flags"] == _capi.PSF_REFINED and sc_at[0]["coarse"]["hyp"] == 1


# ---- group 3

@pytest.mark.parametrize("name", sorted(H.number_range()))
def test_number_range(fref, name):
    """{254, 255}, {0, 1} and {0, 255} at (0, 0) and two opposite corners are FOUND and REFINED; Sbb of the bright pair at (0, 0) exceeds 2^28; a constant
    255 template is NO_TEXTURE and SKIPPED; the bright pair under a 45 degree fine entry runs every shift through the ragged mask"""
    c = H.number_range()[name]
    out = _reference(fref, c)
    _meets(c, out)
    rec, sc = out["fine"]
    p = rec["fine"]
    print(f"{name}: fine flags {p['flags']} n {p['n_overlap']} sa {p['sa']} sb {p['sb']} sab {p['sab']} saa {p['saa']} sbb {p['sbb']} score {p['score']}")
    if name == "bright(0,0)":
        assert p["sbb"] > 1 << 28 and p["saa"] == p["sbb"] and p["n_overlap"] == F.FW * F.FH
    if c.want.get("skipped"):
        assert all(r["flags"] == _capi.PS_NO_TEXTURE for r in (out["coarse"][0], out["oriented"][0]["base"]))
        assert p["flags"] == _capi.PSF_SKIPPED and np.array_equal(sc.view(np.uint64), np.full(sc.shape, H.QNAN64, np.uint64))
    if c.want.get("masked"):
        assert not np.isnan(sc).any() and p["flags"] in (_capi.PSF_LOW_SCORE, _capi.PSF_REFINED)
        assert 64 <= p["n_overlap"] < (F.FW - abs(int(p["sx"]))) * (F.FH - abs(int(p["sy"])))         # fewer pixels than the shift's whole overlap
        assert 254 * 254 * int(p["n_overlap"]) <= p["sbb"] <= 255 * 255 * int(p["n_overlap"]) and 254 * int(p["n_overlap"]) <= p["sb"] <= 255 * int(p["n_overlap"])


# ---- group 4

@pytest.mark.parametrize("name", list(H.single_pixels()))
def test_zero_variance_inside_a_scored_table(fref, name):
    """one pixel of 200 in a template of 77: the coarse stage is FOUND, the fine stage REFINED, and in both tables the NaN set is exactly the set of
    shifts whose overlap does not hold the pixel on both sides, from the overlap formula; the tables hold scored and NaN shifts"""
    c = H.single_pixels()[name]
    out = _reference(fref, c)
    _meets(c, out)
    pt, pi = c.want["pixel"], c.want["image_pixel"]
    coarse = np.array([[H.holds(S.TW, S.TH, (pt[0] // 2, pt[1] // 2), (pi[0] // 2, pi[1] // 2), dx, dy) for dx in range(-S.RX, S.RX + 1)] for dy in range(-S.RY, S.RY + 1)])
    assert np.array_equal(~np.isnan(out["coarse"][1]), coarse) and coarse.any() and not coarse.all()
    cx, cy = 2 * c.want["coarse"][0], 2 * c.want["coarse"][1]
    fine = np.array([[H.holds(F.FW, F.FH, pt, pi, cx + ex, cy + ey) for ex in range(-4, 5)] for ey in range(-4, 5)])
    sc = out["fine"][1][0]
    print(f"{name}: NaN in the coarse table {int((~coarse).sum())} of {coarse.size}, in the fine table {int((~fine).sum())} of {fine.size}")
    assert np.array_equal(~np.isnan(sc), fine) and fine.any()
    # |ex| <= 4 never loses column 4 or 75 of an image that is not moved: those two fine tables are wholly scored, and their moved twins are mixed
    assert fine.all() == (name in ("pixel(4,28)", "pixel(75,28)"))


# ---- group 5

def test_neighbours_in_one_call(fref):
    """the eight pairs of the call are of the four kinds, each with the flags it is built for; a SKIPPED pair's table is quiet NaN in the header's bits
    and its start eight quiet NaNs"""
    cases = H.neighbours()
    assert len(H.batches(dict(enumerate(cases)))) == 1
    flags = []
    for c, kind in zip(cases, H.NEIGHBOUR_KINDS):
        out = _reference(fref, c)
        _meets(c, out)
        rec, sc = out["fine"]
        p = rec["fine"]
        flags.append(int(p["flags"]))
        assert p["flags"] == c.want["flags"], (kind, p["flags"])
        if kind == "skipped":
            assert rec["coarse"]["base"]["flags"] == _capi.PS_LOW_SCORE
            assert np.array_equal(sc.view(np.uint64), np.full(sc.shape, H.QNAN64, np.uint64)) and np.array_equal(p["start_px"].view(np.uint32), F.NAN32)
        elif kind == "nothing":
            assert np.isnan(sc).all() and p["start_px"].tobytes() == rec["coarse"]["base"]["start_px"].tobytes()
        elif kind == "low":
            assert 0.99 < p["score"] < 1.0 and (p["sx"], p["sy"]) == (0, 0)
    assert set(flags) == {_capi.PSF_REFINED, _capi.PSF_SKIPPED, _capi.PSF_NOTHING_SCORED, _capi.PSF_LOW_SCORE}
