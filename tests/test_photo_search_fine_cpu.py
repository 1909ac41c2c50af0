"""The fine stage of the search around the oriented winner and the fine relocalisation (include/hnet.h hnet_op_photo_search_fine,
hnet_sessions_keyframe_relocalise_fine; include/hnet_photo_search_fine.h) on the CPU: the host reference tests/cpp/photo_search_fine_ref.cpp -
the functions the device compiles - against the pyramid's level 2, numpy rotations at the quarter turns, a numpy restatement of the warp, the masked
sums, the order and the record, the hand-built cases, the yawed rows under two tables (the condition of the feature and the gates of the GPU tests), the
kidnapped-and-turned rows under the 12-degree table, and its core under AddressSanitizer + UBSan (tests/cpp/photo_search_fine_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import keyframe_map_util as KM
import photo_align_util as U
import photo_search_fine_util as F
import photo_search_oriented_util as O
import photo_search_util as S
from cuahn_vio_amd import _capi

ROOT = U.ROOT
NAN32 = F.NAN32


@pytest.fixture(scope="module")
def fref(tmp_path_factory):
    return F.build_ref(tmp_path_factory.mktemp("photo_search_fine_ref"))


def _same(a, b, dtype):
    """two records byte for byte, with a message that names the field"""
    for f in dtype.names:
        assert np.atleast_1d(a[f]).tobytes() == np.atleast_1d(b[f]).tobytes(), (f, a[f], b[f])
    assert a.tobytes() == b.tobytes()


def test_level_2_thumbnail_is_the_pyramid_s(fref):
    """the level-2 thumbnail equals two cascaded down4 of the frame, and its own down4 is 7r's level-3 thumbnail"""
    key, views, _ = O.yawed(2)
    for img in (key, views[3]):
        t2 = F.ref_thumb2(fref, img)
        assert np.array_equal(t2, F.np_thumb2(img))
        t = t2.astype(np.int64)
        assert np.array_equal(((t[0::2, 0::2] + t[0::2, 1::2] + t[1::2, 0::2] + t[1::2, 1::2] + 2) >> 2).astype(np.uint8), S.ref_thumbnail(fref, img))
    t2 = F.hand_built()["peak(30,20)"][0]
    assert np.array_equal(F.ref_thumb2(fref, F.expand4(t2)), t2)


def test_identity_and_quarter_turns(fref):
    """the identity warp is the thumbnail under a full mask; 180 degrees is the thumbnail turned; +-90 degrees equal the numpy rotation on the valid
    columns 12 .. 67"""
    t = F.hand_built()["peak(30,20)"][0]
    w, m = F.ref_warp(fref, t, [65536, 0, 0, 65536])
    assert np.array_equal(w, t) and (m == 1).all()
    for deg in (90.0, 180.0, 270.0, -90.0):
        w, m = F.ref_warp(fref, t, O.hyp(fref, deg)["b"][0])
        if deg == 180.0:
            assert (m == 1).all() and np.array_equal(w, t[::-1, ::-1])
            continue
        rot = np.rot90(t, -1 if deg == 90.0 else 1)                  # [80, 56]: its rows 12 .. 67 land on the 56 rows
        assert np.array_equal(m, np.tile((np.arange(80) >= 12) & (np.arange(80) <= 67), (56, 1)).astype(np.uint8))
        assert np.array_equal(w[:, 12:68], rot[12:68, :]) and not w[:, :12].any() and not w[:, 68:].any()


def test_fine_yaw_table(fref):
    """fine_yaw_table against numpy; for odd n_fine its middle column equals yaw_table byte for byte; what it refuses"""
    for first, step, count, n_fine in ((-180.0, 6.0, 60, 5), (-180.0, 12.0, 30, 5), (-36.0, 6.0, 13, 3), (0.0, 15.0, 24, 9), (-180.0, 6.0, 60, 2), (5.0, 7.0, 1, 1)):
        t = F.fine_yaw_table(fref, first, step, count, n_fine)
        if n_fine % 2:
            assert t[:, n_fine // 2].tobytes() == O.yaw_table(fref, first, step, count).tobytes()
        for h in range(count):
            for j in range(n_fine):
                r = np.deg2rad((first + h * step) + (j - (n_fine - 1) / 2.0) * (step / n_fine))
                assert np.allclose(t["a"][h, j], [np.cos(r), -np.sin(r), np.sin(r), np.cos(r)], atol=1e-14)
                assert np.abs(t["b"][h, j] - 65536 * np.linalg.inv(t["a"][h, j].reshape(2, 2)).reshape(4)).max() <= 0.5 + 1e-9
        assert fref.photo_search_fine_ref_table_valid(F._p(t), count, n_fine) == 1
    out = np.zeros((65, 10), F.HYP)
    for bad in ((0.0, 6.0, 0, 5), (0.0, 6.0, 65, 5), (0.0, 6.0, 4, 0), (0.0, 6.0, 4, 10), (float("nan"), 6.0, 4, 5), (0.0, float("inf"), 4, 5)):
        assert fref.photo_search_fine_ref_yaw_table(bad[0], bad[1], bad[2], bad[3], F._p(out)) == 0
    t = F.fine_yaw_table(fref, 0.0, 6.0, 3, 3)
    for field, k, v in (("a", 2, np.nan), ("b", 1, 2 * 65536 + 1)):
        bad = t.copy()
        bad[field][2, 1][k] = v
        assert fref.photo_search_fine_ref_table_valid(F._p(bad), 3, 3) == 0
    assert fref.photo_search_fine_ref_table_valid(None, 3, 3) == 0 and fref.photo_search_fine_ref_table_valid(F._p(t), 3, 10) == 0
    for bad in (dict(radius=-1), dict(radius=5), dict(n_fine=0), dict(n_fine=10), dict(min_score=float("nan")), dict(min_score=1.01), dict(min_score=-1.01)):
        assert fref.photo_search_fine_ref_opts_valid(C.byref(F.fine_opts(fref, **bad))) == 0, bad
    d = F.fine_opts(fref)
    assert (d.radius, d.n_fine, d.min_score) == (3, 5, 0.75) and fref.photo_search_fine_ref_opts_valid(C.byref(d)) == 1


def test_order_is_total(fref):
    """better: the score, then ex^2 + ey^2, then ey, then ex, then j; exactly one of two distinct candidates is better"""
    idx = lambda j, ex, ey: j * 81 + (ey + 4) * 9 + (ex + 4)
    B = fref.photo_search_fine_ref_better
    assert B(0.9, idx(3, 4, 4), 0.8, idx(0, 0, 0)) == 1 and B(0.5, idx(0, 0, 0), 0.8, idx(3, 4, 4)) == 0
    assert B(0.5, idx(2, 1, 0), 0.5, idx(0, 1, 1)) == 1 and B(0.5, idx(2, 1, 0), 0.5, idx(0, 0, 1)) == 1       # radius, then ey
    assert B(0.5, idx(2, -1, 0), 0.5, idx(0, 1, 0)) == 1 and B(0.5, idx(1, 2, -1), 0.5, idx(2, 2, -1)) == 1    # ex, then j
    cands = [idx(j, ex, ey) for j in (0, 4, 8) for ex in (-4, -1, 0, 2) for ey in (-3, 0, 1)]
    for a in cands:
        for b in cands:
            assert B(0.25, a, 0.25, b) + B(0.25, b, 0.25, a) == (0 if a == b else 1)


SCALED = ((0.0, 1.0), (30.0, 0.8), (7.0, 1.25), (-12.0, 1.0))


@pytest.mark.parametrize("n_fine,radius", [(1, 0), (2, 3), (5, 3), (9, 4), (5, 4), (2, 0)])
def test_header_matches_numpy_on_the_pairs(fref, n_fine, radius):
    """the header against the numpy restatement on 7r's 20 pairs under a table with scaled entries: the warp, the masked sums, the order and the record;
    sums, indices and flags exact, scores bit-equal, the coarse part photo_search_oriented_ref's record byte for byte"""
    hyps, o = O.table(fref, *SCALED), S.search_opts()
    fo = F.fine_opts(fref, n_fine=n_fine, radius=radius)
    fine = F.fine_rows(fref, *F.around(SCALED, n_fine, 6.0))
    flags = set()
    for seed in S.SEEDS:
        key, views, _, other = S.cases(seed)
        img2 = np.concatenate([views, other[None]])
        keys = np.stack([key] * 5)
        rec, scores = F.ref_run(fref, keys, img2, o, hyps, fo, fine)
        coarse, _ = O.ref_run(fref, keys, img2, o, hyps)
        t = F.np_thumb2(key)
        for i in range(5):
            assert rec[i]["coarse"].tobytes() == coarse[i].tobytes()
            want, table = F.np_refine(t, F.np_thumb2(img2[i]), coarse[i], o.min_overlap, fo, fine)
            assert np.array_equal(scores[i].view(np.uint64), table.view(np.uint64)), (seed, i)
            _same(rec[i]["fine"], want[0], F.PART)
            flags.add(int(rec[i]["fine"]["flags"]))
    assert _capi.PSF_REFINED in flags and _capi.PSF_SKIPPED in flags


def test_warp_and_sums_match_numpy(fref):
    """the warp under scaled and turned entries and the masked sums at the corners of the shift range against numpy, exactly"""
    key, views, _ = O.yawed(2)
    ta, tb = F.np_thumb2(key), F.np_thumb2(views[1])
    for deg, scale in SCALED + ((33.0, 1.0), (177.0, 0.5), (-131.0, 2.0)):
        b = O.hyp(fref, deg, scale)["b"][0]
        w, m = F.ref_warp(fref, ta, b)
        nw, nm = F.np_warp(ta, b)
        assert np.array_equal(w, nw) and np.array_equal(m, nm) and not w[m == 0].any()
        for sx, sy in ((64, 44), (-64, 44), (64, -44), (-64, -44), (0, 0), (3, -7), (-61, 1)):
            sums, score = F.ref_shift(fref, w, m, tb, sx, sy, 64)
            want = F.np_shift(nw, nm, tb, sx, sy)
            assert tuple(int(x) for x in sums) == want
            ns = S.np_score(want, 64)
            assert (score is None) == (ns is None) and (score is None or score == ns)


@pytest.mark.parametrize("name", sorted(F.hand_built()))
def test_hand_built_cases(fref, name):
    """the header equals the numpy restatement byte for byte, and the flags, the tie order and the start are the expected ones"""
    fa, fb, o, hyps, fo, fine = F.case_tables(fref, name)
    rec, scores = F.ref_run(fref, fa[None], fb[None], o, hyps, fo, fine)
    a, b = F.hand_built()[name][:2]
    c, p = rec[0]["coarse"], rec[0]["fine"]
    want, table = F.np_refine(a, b, c, o.min_overlap, fo, fine)
    assert np.array_equal(scores[0].view(np.uint64), table.view(np.uint64))
    _same(p, want[0], F.PART)
    assert not p["pad0"] and not p["pad1"]
    if name == "peak(30,20)":
        assert (c["base"]["flags"], c["base"]["dx"], c["base"]["dy"]) == (_capi.PS_FOUND, 30, 20)
        assert not np.isnan(scores[0, 0]).any() and not np.isnan(scores[0, 0, 8, 8])           # (64, 44) is scored at 4 * 16 pixels
        assert (p["flags"], p["j"], p["ex"], p["ey"], p["sx"], p["sy"], p["n_overlap"]) == (_capi.PSF_REFINED, 0, 0, 0, 60, 40, 20 * 16) and p["score"] == 1.0
        assert np.array_equal(p["start_px"], np.tile(np.array([240.0, 160.0], np.float32), 4))
    elif name == "same-fine-entry-twice":
        assert np.array_equal(scores[0, 1].view(np.uint64), scores[0, 2].view(np.uint64)) and (p["flags"], p["j"], p["sx"], p["sy"]) == (_capi.PSF_REFINED, 1, 6, 0)
    elif name == "tie-between-shifts":
        s = scores[0, 0]
        assert s[4, 3] == s[4, 5] == np.nanmax(s) and s[4, 4] < s[4, 3]
        assert (p["flags"], p["ex"], p["ey"]) == (_capi.PSF_REFINED, -1, 0) and p["score"] == s[4, 3]
    elif name == "coarse-low-score":
        assert c["base"]["flags"] == _capi.PS_LOW_SCORE and p["flags"] == _capi.PSF_SKIPPED and np.isnan(scores).all()
        assert np.array_equal(p["start_px"].view(np.uint32), NAN32) and (p["j"], p["score"]) == (-1, -1.0) and not p["a"].any()
    elif name == "scale-half-scores-nothing":
        w, m = F.ref_warp(fref, a, fine["b"][0, 0])
        assert int(m.sum()) == 40 * 28 < 4 * o.min_overlap and np.isnan(scores).all()
        assert c["base"]["flags"] == _capi.PS_FOUND and p["flags"] == _capi.PSF_NOTHING_SCORED and (p["j"], p["score"]) == (-1, -1.0)
        assert p["start_px"].tobytes() == c["base"]["start_px"].tobytes()
    elif name == "min-score-one":
        assert c["base"]["flags"] == _capi.PS_FOUND and p["flags"] == _capi.PSF_LOW_SCORE and 0.99 < p["score"] < 1.0 and (p["j"], p["ex"], p["ey"]) == (0, 0, 0)
        assert p["start_px"].tobytes() == c["base"]["start_px"].tobytes() and np.array_equal(p["a"], [1.0, 0.0, 0.0, 1.0])


def _rows(fref, table, n_fine=5, radius=3):
    """the 20 yawed rows under a table -> the list of (seed, row, record, coarse error, fine error)"""
    hyps, fine = O.yaw_table(fref, *table), F.fine_yaw_table(fref, *table, n_fine)
    o, fo = S.search_opts(), F.fine_opts(fref, n_fine=n_fine, radius=radius)
    out = []
    for seed in S.SEEDS:
        key, views, poses = O.yawed(seed)
        rec, _ = F.ref_run(fref, np.stack([key] * len(views)), views, o, hyps, fo, fine)
        for i in range(len(views)):
            out.append((seed, i, rec[i], S.worst_px(rec[i]["coarse"]["base"]["start_px"], poses[i]), S.worst_px(rec[i]["fine"]["start_px"], poses[i])))
    return out


@pytest.mark.parametrize("table,measured,gate", [(F.TABLE_60, F.FINE_START_60, F.GATE_FINE_60), (F.TABLE_30, F.FINE_START_30, F.GATE_FINE_30)])
def test_the_yawed_rows(fref, table, measured, gate):
    """7s's 20 yawed rows (seeds 1, 2, 5, 11 x YAW_ROWS) under (60 x 6 degrees, n_fine 5, r 3) and (30 x 12 degrees from -180, n_fine 5, r 3).  A condition
    and not a measurement: every row is REFINED and its fine start is strictly closer to the truth than its coarse start.  The worst fine start printed
    here is the measured value of photo_search_fine_util, whose gate is twice it and below the alignment's basin of 24 px."""
    rows = _rows(fref, table)
    assert len(rows) == 20
    for seed, i, r, ec, ef in rows:
        p = r["fine"]
        print(f"table {table[2]} x {table[1]:.0f} deg, seed {seed} yaw {O.YAW_ROWS[i][0]:6.1f}: coarse entry {r['coarse']['hyp']} score {r['coarse']['base']['score']:.3f} start "
              f"{ec:.2f} px | fine j {p['j']} e ({p['ex']}, {p['ey']}) score {p['score']:.3f} flags {p['flags']} start {ef:.2f} px")
    worst_c, worst_f = max(r[3] for r in rows), max(r[4] for r in rows)
    print(f"table {table[2]} x {table[1]:.0f} deg: coarse start worst {worst_c:.2f} px, fine start worst {worst_f:.2f} px, gate {gate:.2f} px, fine score "
          f"{min(r[2]['fine']['score'] for r in rows):.3f} .. {max(r[2]['fine']['score'] for r in rows):.3f}")
    for seed, i, r, ec, ef in rows:
        assert r["coarse"]["base"]["flags"] == _capi.PS_FOUND and r["fine"]["flags"] == _capi.PSF_REFINED, (seed, i)
        assert ef < ec, (seed, i, ec, ef)
        assert np.array_equal(r["fine"]["start_px"], F.np_start(r["fine"]["a"], int(r["fine"]["sx"]), int(r["fine"]["sy"])))
    assert worst_f <= measured + 0.005 and worst_f > measured - 0.005       # the gate is twice this measurement, not wider
    assert gate < O.BASIN_PX


def test_kidnapped_and_turned_rows_under_the_12_degree_table(fref):
    """the host relocalise with the fine stage on the kidnapped-and-turned rows (turned, turned_map) under the 30 x 12 degree table, seeds 1, 2, 5, 11: the
    verdicts and the distances are printed beside the 60-entry oriented relocalise's; every row is recovered inside 7s's gates"""
    hyps, fine, fo = O.yaw_table(fref, *F.TABLE_30), F.fine_yaw_table(fref, *F.TABLE_30, 5), F.fine_opts(fref)
    for seed in S.SEEDS:
        ses = F.RefSession(fref, 0)
        lost, rl, nxt = O.run_turned(seed, ses.track, lambda f, o: ses.relocalise_fine(f, o, hyps, fo, fine))
        _, poses, _ = O.turned(seed)
        b, p = rl["base"], rl["fine"]
        e_rl, e_next = S.worst_px(b["rv"]["key_px"], poses[1]), S.worst_px(nxt["key_px"], poses[2])
        print(f"kidnapped and turned, 30 x 12, seed {seed}: coarse entry {b['search']['hyp']} score {b['search']['base']['score']:.3f} start "
              f"{S.worst_px(b['search']['base']['start_px'], poses[1]):.2f} px; fine flags {p['flags']} j {p['j']} score {p['score']:.3f} start "
              f"{S.worst_px(p['start_px'], poses[1]):.2f} px; relocalise flags {b['rv']['flags']} at {e_rl:.4f} px; next track flags {nxt['flags']} at {e_next:.4f} px")
        assert p["flags"] == _capi.PSF_REFINED and b["rv"]["flags"] == _capi.RL_RETRACKED and b["target"] == _capi.RL_TARGET_HELD and not (nxt["flags"] & _capi.KF_LOST)
        assert b["rv"]["start_px"].tobytes() == p["start_px"].tobytes() and e_rl <= O.GATE_TURNED
        ses = F.RefSession(fref, S.CAPACITY)
        far, rm = O.run_turned_map(seed, ses.track, lambda f, o: ses.relocalise_fine(f, o, hyps, fo, fine))
        _, _, pose = O.turned_map(seed)
        b, p = rm["base"], rm["fine"]
        e_after = KM.worst_px(b["rv"]["h_origin_curr"], pose)
        print(f"kidnapped and turned with a map, 30 x 12, seed {seed}: searched {b['n_searched']}, found {b['n_found']}, target {b['target']}, coarse score "
              f"{b['search']['base']['score']:.3f}; fine flags {p['flags']} score {p['score']:.3f}; relocalise flags {b['rv']['flags']}; h_origin_curr at {e_after:.4f} px")
        assert far["flags"] & _capi.KF_LOST and p["flags"] == _capi.PSF_REFINED and b["rv"]["flags"] == _capi.RL_ATTACHED and e_after <= O.GATE_TURNED_MAP


def test_relocalise_without_a_pick_is_skipped(fref):
    """a fine relocalise that finds nothing leaves the state as it was; the fine part is SKIPPED with a quiet-NaN start and the base is the oriented call's"""
    frames, _, _ = O.turned(1)
    _, _, _, other = S.cases(1)
    hyps, fine, fo = O.yaw_table(fref, *F.TABLE_30), F.fine_yaw_table(fref, *F.TABLE_30, 5), F.fine_opts(fref)
    ses, twin = F.RefSession(fref, 0), F.RefSession(fref, 0)
    for s in (ses, twin):
        s.track(frames[0], None, O.K.opts(**S.KIDNAP_TRACK))
    before = ses.snapshot()
    none = ses.relocalise_fine(other, S.reloc_opts(), hyps, fo, fine)
    assert none["base"].tobytes() == twin.relocalise_oriented(other, S.reloc_opts(), hyps).tobytes() and ses.snapshot() == before
    assert none["base"]["rv"]["flags"] == _capi.RL_NO_CANDIDATE and none["fine"]["flags"] == _capi.PSF_SKIPPED
    assert np.array_equal(none["fine"]["start_px"].view(np.uint32), NAN32) and none["fine"]["j"] == -1


def test_photo_search_fine_check_under_asan_ubsan(tmp_path):
    """the reference core on heap thumbnails of exactly 4 480 bytes: every shift at r = 4 at the four corners of the coarse range, a 9-entry row, the
    hand-built kinds and one relocalise under AddressSanitizer + UBSan: a stand-alone program; nothing loaded into python is sanitized"""
    exe = str(tmp_path / "photo_search_fine_check_san.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *U.HOST_FLAGS,
                    os.path.join(ROOT, "tests", "cpp", "photo_search_fine_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "photo_search_fine_check: ok" in r.stdout
