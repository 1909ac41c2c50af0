"""The coarse search under a table of orientation hypotheses and the oriented relocalisation (include/hnet.h hnet_op_photo_search_oriented,
hnet_sessions_keyframe_relocalise_oriented; include/hnet_photo_search_oriented.h) on the CPU: the host reference
tests/cpp/photo_search_oriented_ref.cpp - the functions the device compiles - against 7r's reference under the identity, numpy rotations at the quarter
turns, a numpy restatement of the warp, the masked sums, the per-entry search and the winner, the hand-built cases, the yawed views of the wide canvas, the
kidnapped-and-turned rows that set the gates of the GPU tests, and its core under AddressSanitizer + UBSan (tests/cpp/photo_search_oriented_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import keyframe_map_util as KM
import keyframe_util as K
import photo_align_util as U
import photo_search_oriented_util as O
import photo_search_util as S
from cuahn_vio_amd import _capi

ROOT = U.ROOT
NAN32 = np.array([0x7FC00000] * 8, np.uint32)


@pytest.fixture(scope="module")
def oref(tmp_path_factory):
    return O.build_ref(tmp_path_factory.mktemp("photo_search_oriented_ref"))


def _same(a, b, dtype):
    """two records byte for byte, with a message that names the field"""
    for f in dtype.names:
        assert np.atleast_1d(a[f]).tobytes() == np.atleast_1d(b[f]).tobytes(), f
    assert a.tobytes() == b.tobytes()


def test_tables(oref):
    """make_hyp and yaw_table: A and round(65536 A^-1), exact at the quarter turns, the limits of the scale, the count and what a call refuses"""
    t = O.yaw_table(oref)
    assert len(t) == 60 and np.array_equal(t["b"][30], [65536, 0, 0, 65536]) and np.array_equal(t["a"][30], [1.0, 0.0, 0.0, 1.0])
    assert np.array_equal(t["b"][45], [0, 65536, -65536, 0]) and np.array_equal(t["b"][0], [-65536, 0, 0, -65536]) and np.array_equal(t["b"][15], [0, -65536, 65536, 0])
    for k in range(60):
        r = np.deg2rad(-180.0 + 6.0 * k)
        assert np.allclose(t["a"][k], [np.cos(r), -np.sin(r), np.sin(r), np.cos(r)], atol=1e-15)
        inv = np.linalg.inv(t["a"][k].reshape(2, 2)).reshape(4)
        assert np.abs(t["b"][k] - 65536 * inv).max() <= 0.5 + 1e-9
    h = O.hyp(oref, 30.0, 0.8)
    assert np.abs(h["b"][0] - 65536 * np.linalg.inv(h["a"][0].reshape(2, 2)).reshape(4)).max() <= 0.5 + 1e-9
    out = np.zeros(65, O.HYP)
    for bad in ((0.0, 0.49), (0.0, 2.01), (float("nan"), 1.0), (float("inf"), 1.0), (0.0, float("nan"))):
        assert oref.photo_search_oriented_ref_make_hyp(bad[0], bad[1], O._p(out)) == 0 and not out.tobytes().strip(b"\0")
    assert oref.photo_search_oriented_ref_yaw_table(-180.0, 6.0, 0, O._p(out)) == 0 and oref.photo_search_oriented_ref_yaw_table(-180.0, 6.0, 65, O._p(out)) == 0
    assert oref.photo_search_oriented_ref_table_valid(O._p(t), 60) == 1 and oref.photo_search_oriented_ref_table_valid(O._p(t), 0) == 0
    assert oref.photo_search_oriented_ref_table_valid(O._p(out), 65) == 0
    for field, k, v in (("a", 2, np.nan), ("a", 0, np.inf), ("b", 1, 2 * 65536 + 1), ("b", 3, -2 * 65536 - 1)):
        bad = t[:3].copy()
        bad[field][1][k] = v
        assert oref.photo_search_oriented_ref_table_valid(O._p(bad), 3) == 0, (field, k, v)
    edge = O.hyp(oref, 0.0, 0.5)
    assert edge["b"][0][0] == 2 * 65536 and oref.photo_search_oriented_ref_table_valid(O._p(edge), 1) == 1


@pytest.mark.parametrize("seed", S.SEEDS)
def test_identity_is_the_plain_search(oref, seed):
    """the identity entry's warped template is the thumbnail under a full mask, and a table of only the identity gives photo_search_ref's record in the
    first 96 bytes and its score table, on the 5 pairs of the seed (20 over the seeds)"""
    key, views, _, other = S.cases(seed)
    o, ident = S.search_opts(), O.table(oref, *O.IDENTITY)
    t = S.ref_thumbnail(oref, key)
    w, m = O.ref_warp(oref, t, ident["b"][0])
    assert np.array_equal(w, t) and (m == 1).all()
    img2 = np.concatenate([views, other[None]])
    plain, pscores = S.ref_run(oref, np.stack([key] * 5), img2, o)
    rec, scores = O.ref_run(oref, np.stack([key] * 5), img2, o, ident)
    assert scores.shape == (5, 1, S.NSY, S.NSX) and np.array_equal(scores[:, 0].view(np.uint64), pscores.view(np.uint64))
    for i in range(5):
        assert rec[i].tobytes()[:96] == plain[i].tobytes()
        assert (rec[i]["hyp"], rec[i]["n_scored"], rec[i]["hyp2"], rec[i]["score2"]) == (0, 1, -1, -1.0) and np.array_equal(rec[i]["a"], ident["a"][0])
        assert not rec[i]["pad"].any() and rec[i]["pad0"] == 0


@pytest.mark.parametrize("name", sorted(S.hostile()))
def test_identity_on_the_hostile_thumbnails(oref, name):
    a, b, o, _ = S.hostile()[name]
    plain, pscores = S.ref_search(oref, a, b, o)
    rec, scores, per = O.ref_search(oref, a, b, o, O.table(oref, *O.IDENTITY))
    assert rec[0].tobytes()[:96] == plain[0].tobytes() and np.array_equal(scores[0].view(np.uint64), pscores.view(np.uint64))
    scored = plain["flags"][0] != _capi.PS_NO_TEXTURE
    assert (rec["hyp"][0], rec["n_scored"][0]) == ((0, 1) if scored else (-1, 0)) and np.array_equal(rec["a"][0], [1.0, 0, 0, 1.0] if scored else [0.0] * 4)


def test_quarter_turns_are_numpy_rotations(oref):
    """the warped thumbnail at 90, 180 and 270 degrees equals the numpy rotation on the valid region, exactly: x' = c + R (x - c), y down, so a turn by +90
    degrees takes the thumbnail's column u to row u of the result"""
    t = S.hostile()["peak(30,20)"][0]
    for deg in (90.0, 180.0, 270.0, -90.0):
        w, m = O.ref_warp(oref, t, O.hyp(oref, deg)["b"][0])
        if deg == 180.0:
            assert (m == 1).all() and np.array_equal(w, t[::-1, ::-1])
            continue
        rot = np.rot90(t, -1 if deg == 90.0 else 1)                  # [40, 28]: the whole thumbnail turned; its rows 6 .. 33 land on the 28 rows
        assert np.array_equal(m, np.tile((np.arange(40) >= 6) & (np.arange(40) <= 33), (28, 1)).astype(np.uint8))
        assert np.array_equal(w[:, 6:34], rot[6:34, :]) and not w[:, :6].any() and not w[:, 34:].any()


TABLES = {
    1: ((-30.0, 1.0),),
    2: ((12.0, 1.0), (-170.0, 0.7)),
    5: O.TABLE5,
}


@pytest.mark.parametrize("n_hyp", [1, 2, 5, 64])
def test_header_matches_numpy(oref, n_hyp):
    """the header against the numpy restatement of the warp, the masked sums, the score, the per-entry best and second and the winner: sums, shifts, flags,
    indices and n_overlap exact, every score bit-equal.  Tables of 1, 2, 5 and 64 entries (the last at radii 10 x 6, which keeps the restatement quick)"""
    seed = 2
    key, views, _ = O.yawed(seed)
    ta, tb = S.np_thumbnail(key), S.np_thumbnail(views[1])
    if n_hyp == 64:
        hyps, o = O.yaw_table(oref, -180.0, 5.625, 64), S.search_opts(radius_x=10, radius_y=6)
    else:
        hyps, o = O.table(oref, *TABLES[n_hyp]), S.search_opts()
    rec, scores, per = O.ref_search(oref, ta, tb, o, hyps)
    want, table, wper = O.np_search(ta, tb, o, hyps)
    for h in range(n_hyp):
        w, m = O.ref_warp(oref, ta, hyps["b"][h])
        nw, nm = O.np_warp(ta, hyps["b"][h])
        assert np.array_equal(w, nw) and np.array_equal(m, nm) and not w[m == 0].any()
        assert np.array_equal(scores[h].view(np.uint64), table[h].view(np.uint64)), h
        _same(per[h], wper[h], S.SEARCH)
        dx, dy = int(wper["dx"][h]), int(wper["dy"][h])
        sums, score = O.ref_shift(oref, w, m, tb, dx, dy, o.min_overlap)
        assert tuple(int(x) for x in sums) == O.np_shift(nw, nm, tb, dx, dy)
        if wper["flags"][h] != _capi.PS_NO_TEXTURE:
            assert score == wper["score"][h]
    _same(rec[0], want[0], O.OREC)
    if n_hyp == 64:
        assert rec["base"]["flags"][0] == _capi.PS_FOUND and abs(O.wrap_deg(O.hyp_deg(hyps[rec["hyp"][0]]) - O.YAW_ROWS[1][0])) <= 5.625


@pytest.mark.parametrize("name", sorted(O.hand_built()))
def test_hand_built_cases(oref, name):
    """the header equals the numpy restatement byte for byte, and the winner, the tie order and the flags are the expected ones"""
    a, b, o, entries = O.hand_built()[name]
    hyps = O.table(oref, *entries)
    rec, scores, per = O.ref_search(oref, a, b, o, hyps)
    want, table, _ = O.np_search(a, b, o, hyps)
    assert np.array_equal(scores.view(np.uint64), table.view(np.uint64))
    _same(rec[0], want[0], O.OREC)
    r = rec[0]
    if name == "same-matrix-twice":
        assert (r["hyp"], r["hyp2"], r["n_scored"]) == (1, 2, 3) and r["score2"] == r["base"]["score"] and per[1].tobytes() == per[2].tobytes()
        assert (r["base"]["dx"], r["base"]["dy"], r["base"]["flags"]) == (3, 0, _capi.PS_FOUND)
    elif name == "scale-half-scores-nothing":
        w, m = O.ref_warp(oref, a, hyps["b"][0])
        assert int(m.sum()) == 280 < o.min_overlap and np.isnan(scores[0]).all() and per["flags"][0] == _capi.PS_NO_TEXTURE
        assert (r["hyp"], r["hyp2"], r["n_scored"], r["score2"], r["base"]["flags"]) == (1, -1, 1, -1.0, _capi.PS_FOUND)
    elif name in ("only-scale-half", "constant-template"):
        assert np.isnan(scores).all() and (r["hyp"], r["hyp2"], r["n_scored"], r["score2"]) == (-1, -1, 0, -1.0) and not r["a"].any()
        assert r["base"]["flags"] == _capi.PS_NO_TEXTURE and np.array_equal(r["base"]["start_px"].view(np.uint32), NAN32)
        assert (r["base"]["dx"], r["base"]["dy"], r["base"]["n_overlap"], r["base"]["score"], r["base"]["second"]) == (0, 0, 0, -1.0, -1.0)
    elif name == "edge-peak-under-90":
        assert (r["hyp"], r["base"]["dx"], r["base"]["dy"], r["base"]["n_overlap"], r["base"]["flags"]) == (1, 30, 20, 32, _capi.PS_FOUND)
        assert abs(r["base"]["score"] - 1.0) < 1e-15 and np.array_equal(r["base"]["start_px"], O.np_start(hyps["a"][1], 30, 20))


def test_the_yawed_rows(oref):
    """seeds 1, 2, 5, 11; the keyframe's view of the wide canvas against views yawed 20, 33, 58, 177 and -131 degrees about the frame centre and moved by
    up to 40 x 30 px; the table is 60 x 6 degrees.  On every row 7r's search is not FOUND and the oriented search is FOUND on an entry within one step
    of the truth, its start inside the alignment's basin of 24 px.  Printed per row: the score, the second, the runner-up, the best score of an entry two
    or more steps away, and the start's worst corner error (DESIGN 7s records them beside the prototype's)."""
    tab, o = O.yaw_table(oref), S.search_opts()
    span = dict(score=[9.0, -9.0], second=[9.0, -9.0], runner=[9.0, -9.0], far=[9.0, -9.0], start=[9e9, -9.0], plain=[9.0, -9.0])

    def note(k, v):
        span[k] = [min(span[k][0], v), max(span[k][1], v)]

    for seed in S.SEEDS:
        key, views, poses = O.yawed(seed)
        keys = np.stack([key] * len(views))
        plain, _ = S.ref_run(oref, keys, views, o)
        rec, scores = O.ref_run(oref, keys, views, o, tab)
        for i, (deg, t) in enumerate(O.YAW_ROWS):
            r, b = rec[i], rec[i]["base"]
            off = abs(O.wrap_deg(O.hyp_deg(tab[r["hyp"]]) - deg))
            err = S.worst_px(b["start_px"], poses[i])
            away = np.array([abs(O.wrap_deg(O.hyp_deg(tab[h]) - O.hyp_deg(tab[r["hyp"]]))) >= 2 * O.STEP_DEG - 1e-9 for h in range(len(tab))])
            far = float(np.nanmax(scores[i][away]))
            print(f"seed {seed} yaw {deg:6.1f} t {t}: 7r flags {plain[i]['flags']} score {plain[i]['score']:.3f} | entry {r['hyp']} ({O.hyp_deg(tab[r['hyp']]):6.1f} deg) shift "
                  f"({b['dx']}, {b['dy']}) score {b['score']:.3f} second {b['second']:.3f} runner-up {r['score2']:.3f} (entry {r['hyp2']}) far {far:.3f} start {err:.2f} px")
            assert plain[i]["flags"] != _capi.PS_FOUND
            assert b["flags"] == _capi.PS_FOUND and off <= O.STEP_DEG + 1e-9 and err <= O.BASIN_PX
            assert np.array_equal(b["start_px"], O.np_start(tab["a"][r["hyp"]], int(b["dx"]), int(b["dy"]))) and r["n_scored"] == len(tab)
            for k, v in (("score", b["score"]), ("second", b["second"]), ("runner", r["score2"]), ("far", far), ("start", err), ("plain", plain[i]["score"])):
                note(k, float(v))
    print("over the 20 rows: " + ", ".join(f"{k} {v[0]:.3f} .. {v[1]:.3f}" for k, v in span.items()))


def test_rejected_and_candidate_less_calls_change_nothing(oref):
    """a whole oriented relocalise on the host that finds nothing (an unrelated frame) or is rejected (max_closure_px = 1e-3) leaves the state, the
    keyframe, the map state, the entries and the images byte for byte, with and without a map; the record says why"""
    seed = 1
    frames, _, _ = O.turned(seed)
    _, _, _, other = S.cases(seed)
    tab = O.yaw_table(oref)
    for capacity in (0, S.CAPACITY):
        ses = O.RefSession(oref, capacity)
        to = K.opts(**S.KIDNAP_TRACK)
        ses.track(frames[0], None, to)
        ses.track(frames[1], None, to)
        before = ses.snapshot()
        none = ses.relocalise_oriented(other, S.reloc_opts(), tab)
        assert none["rv"]["flags"] == _capi.RL_NO_CANDIDATE and none["target"] == _capi.RL_TARGET_NONE and none["n_found"] == 0 and none["n_searched"] >= 1
        assert not none["rv"]["rec"].tobytes().strip(b"\0") and not none["search"].tobytes().strip(b"\0")
        assert np.array_equal(none["rv"]["start_px"].view(np.uint32), NAN32) and ses.snapshot() == before
        rej = ses.relocalise_oriented(frames[1], S.reloc_opts(max_closure_px=1e-3, min_overlap=O.TURNED_MIN_OVERLAP), tab)
        assert rej["rv"]["flags"] == _capi.RL_CLOSURE_ABOVE_MAX and rej["target"] == _capi.RL_TARGET_HELD and rej["search"]["base"]["flags"] == _capi.PS_FOUND
        assert ses.snapshot() == before


def test_kidnapped_and_turned_rows(oref):
    """the host reference on 7r's two kidnapped rows with the lost frame also turned by 33 degrees, seeds 1, 2, 5, 11.  The plain relocalise answers
    NO_CANDIDATE; the oriented one is RETRACKED on the held keyframe (the next track with the true step is TRACKED), and with a map ATTACHED to a stored
    keyframe.  The gates of photo_search_oriented_util are twice the worst error printed here.  At the relocalise's default min_overlap of 0.5 the first
    row's seed 5 is rejected LOW_OVERLAP (49.6 % of the keyframe is in view): the row passes 0.45 (photo_search_oriented_util.TURNED_MIN_OVERLAP)."""
    tab = O.yaw_table(oref)
    worst, worst_map = 0.0, 0.0
    for seed in S.SEEDS:
        ses = O.RefSession(oref, 0)
        _, plain, _ = O.run_turned(seed, ses.track, ses.relocalise)
        assert plain["rv"]["flags"] == _capi.RL_NO_CANDIDATE and plain["n_found"] == 0
        ses = O.RefSession(oref, 0)
        lost, rl, nxt = O.run_turned(seed, ses.track, lambda f, o: ses.relocalise_oriented(f, o, tab))
        _, poses, _ = O.turned(seed)
        e_lost, e_rl, e_next = S.worst_px(lost["key_px"], poses[1]), S.worst_px(rl["rv"]["key_px"], poses[1]), S.worst_px(nxt["key_px"], poses[2])
        print(f"kidnapped and turned, seed {seed}: track flags {lost['flags']} at {e_lost:.2f} px; entry {rl['search']['hyp']} shift ({rl['search']['base']['dx']}, "
              f"{rl['search']['base']['dy']}) score {rl['search']['base']['score']:.3f} start {S.worst_px(rl['search']['base']['start_px'], poses[1]):.2f} px; relocalise "
              f"flags {rl['rv']['flags']} overlap {rl['rv']['overlap']:.3f} at {e_rl:.4f} px; next track flags {nxt['flags']} at {e_next:.4f} px")
        assert (lost["flags"] & _capi.KF_LOST) or e_lost > O.BEFORE_RATIO * O.GATE_TURNED
        assert rl["rv"]["flags"] == _capi.RL_RETRACKED and rl["target"] == _capi.RL_TARGET_HELD and not (nxt["flags"] & _capi.KF_LOST)
        assert np.array_equal(ses.state["key_px"][0], nxt["key_px"])
        worst = max(worst, e_rl)
        ses = O.RefSession(oref, S.CAPACITY)
        _, plain = O.run_turned_map(seed, ses.track, ses.relocalise)
        assert plain["rv"]["flags"] == _capi.RL_NO_CANDIDATE and plain["n_found"] == 0 and plain["n_searched"] >= 2
        ses = O.RefSession(oref, S.CAPACITY)
        far, rm = O.run_turned_map(seed, ses.track, lambda f, o: ses.relocalise_oriented(f, o, tab))
        _, _, pose = O.turned_map(seed)
        e_before, e_after = KM.worst_px(rm["rv"]["h_origin_before"], pose), KM.worst_px(rm["rv"]["h_origin_curr"], pose)
        print(f"kidnapped and turned with a map, seed {seed}: track flags {far['flags']}; searched {rm['n_searched']}, found {rm['n_found']}, target {rm['target']}, "
              f"entry {rm['search']['hyp']} score {rm['search']['base']['score']:.3f}; h_origin_curr {e_before:.3f} px -> {e_after:.4f} px")
        assert far["flags"] & _capi.KF_LOST and rm["rv"]["flags"] == _capi.RL_ATTACHED and rm["target"] >= 0 and rm["rv"]["slot"] == rm["target"]
        assert e_before >= O.BEFORE_RATIO * O.GATE_TURNED_MAP
        assert ses.mstate["cur_slot"][0] == rm["target"] and np.array_equal(ses.state["h_origin_key"][0], ses.entries["h_origin_key"][rm["target"]])
        worst_map = max(worst_map, e_after)
    print(f"worst after the oriented relocalise: kidnapped and turned {worst:.5f} px, with a map {worst_map:.5f} px")
    assert worst <= O.GATE_TURNED / 2 and worst_map <= O.GATE_TURNED_MAP / 2
    assert worst > 0.9 * O.GATE_TURNED / 2 and worst_map > 0.9 * O.GATE_TURNED_MAP / 2        # the gates are these measurements, not wider


def test_photo_search_oriented_check_under_asan_ubsan(tmp_path):
    """the reference core, every shift of the range under three entries on heap thumbnails, a 64-entry table, the hand-built cases and two relocalises
    under AddressSanitizer + UBSan: a stand-alone program; nothing loaded into python is sanitized"""
    exe = str(tmp_path / "photo_search_oriented_check_san.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *U.HOST_FLAGS,
                    os.path.join(ROOT, "tests", "cpp", "photo_search_oriented_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "photo_search_oriented_check: ok" in r.stdout
