"""The coarse search over integer translations and the relocalisation (include/hnet.h hnet_op_photo_search, hnet_sessions_keyframe_relocalise;
include/hnet_photo_search.h, include/hnet_keyframe_reloc.h) on the CPU: the host reference tests/cpp/photo_search_ref.cpp - the functions the
device compiles - against level 3 of the pyramid reference, a numpy restatement of the sums, the score and the pick, the views of the wide canvas, the
hand-built thumbnails, decide_relocalise reason by reason, the kidnapped rows that set the gates of the GPU tests, and its core under AddressSanitizer +
UBSan (tests/cpp/photo_search_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import keyframe_map_util as KM
import keyframe_util as K
import photo_align_pyr_util as P
import photo_align_util as U
import photo_search_util as S
from cuahn_vio_amd import _capi

ROOT = U.ROOT
NAN32 = np.array([0x7FC00000] * 8, np.uint32)


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return S.build_ref(tmp_path_factory.mktemp("photo_search_ref"))


def _same_record(a, b):
    """two search records byte for byte, with a message that names the field"""
    for f in S.SEARCH.names:
        assert np.atleast_1d(a[f]).tobytes() == np.atleast_1d(b[f]).tobytes(), f
    assert a.tobytes() == b.tobytes()


def test_layouts_and_default_opts(sref):
    o = _capi.PhotoSearchOpts()
    sref.photo_search_ref_default_opts(C.byref(o))
    assert bytes(o) == bytes(S.search_opts()) and (o.radius_x, o.radius_y, o.min_overlap, o.min_score, o.min_margin) == (30, 20, 140, 0.75, 0.1)
    r = _capi.KeyframeRelocOpts()
    sref.photo_search_ref_reloc_default_opts(C.byref(r))
    assert bytes(r) == bytes(S.reloc_opts(max_iterations=r.align.base.max_iterations)) and r.levels == 4 and r.min_overlap == 0.5
    assert sref.photo_search_ref_opts_valid(C.byref(o)) == 1 and sref.photo_search_ref_reloc_opts_valid(C.byref(r)) == 1
    for kw in (dict(radius_x=-1), dict(radius_x=31), dict(radius_y=-1), dict(radius_y=21), dict(min_overlap=15), dict(min_overlap=1121), dict(min_score=-1.5),
               dict(min_score=1.5), dict(min_score=float("nan")), dict(min_margin=-0.5), dict(min_margin=2.5), dict(min_margin=float("nan"))):
        bad = S.search_opts(**kw)
        assert sref.photo_search_ref_opts_valid(C.byref(bad)) == 0, kw
        rb = S.reloc_opts(search=bad)
        assert sref.photo_search_ref_reloc_opts_valid(C.byref(rb)) == 0, kw
    for kw in (dict(levels=0), dict(levels=5), dict(min_overlap=-0.1), dict(min_overlap=1.1), dict(max_mse=-1.0), dict(max_closure_px=float("inf"))):
        rb = S.reloc_opts(**kw)
        assert sref.photo_search_ref_reloc_opts_valid(C.byref(rb)) == 0, kw
    for kw in (dict(radius_x=0, radius_y=0), dict(min_overlap=16), dict(min_overlap=1120), dict(min_score=-1.0, min_margin=0.0), dict(min_score=1.0, min_margin=2.0)):
        ok = S.search_opts(**kw)
        assert sref.photo_search_ref_opts_valid(C.byref(ok)) == 1, kw


@pytest.mark.parametrize("seed", S.SEEDS)
def test_thumbnail_is_level_3(sref, seed):
    """bit for bit level 3 of photo_align_pyr_ref.cpp's pyramid (the library holds it) and of the numpy cascade, on a view, and at the ends of the range"""
    key, views, _, _ = S.cases(seed)
    vv, uu = np.meshgrid(np.arange(224), np.arange(320), indexing="ij")
    for img in (key, views[seed % 4], np.full((224, 320), 255, np.uint8), (((uu + vv) & 1) * 255).astype(np.uint8)):
        t = S.ref_thumbnail(sref, img)
        assert np.array_equal(t, P.split_pyramid(P.ref_pyramid(sref, img)[0])[2])
        assert np.array_equal(t, S.np_thumbnail(img)) and np.array_equal(t, P.numpy_pyramid(img)[2])
    th = S.hostile()["peak(30,20)"][1]
    assert np.array_equal(S.ref_thumbnail(sref, S.expand(th)), th)


@pytest.mark.parametrize("seed", S.SEEDS)
def test_search_matches_numpy_on_the_views(sref, seed):
    """the header against the numpy restatement over the full range, per view and on the unrelated frame: sums, shift, flags and n_overlap exact, every
    score of the table bit-equal; the shift is within one level-3 pixel of -t / 8 and FOUND at the defaults; the unrelated frame is LOW_SCORE"""
    key, views, _, other = S.cases(seed)
    o = S.search_opts()
    recs, scores = S.ref_run(sref, np.stack([key] * 5), np.concatenate([views, other[None]]), o)
    ta = S.np_thumbnail(key)
    for i in range(5):
        tb = S.np_thumbnail(views[i] if i < 4 else other)
        want, table = S.np_search(ta, tb, o)
        assert np.array_equal(scores[i].view(np.uint64), table.view(np.uint64))
        _same_record(recs[i], want[0])
        again, _ = S.ref_search(sref, ta, tb, o)
        _same_record(again[0], want[0])
        sums, score = S.ref_shift(sref, ta, tb, int(want["dx"][0]), int(want["dy"][0]), o.min_overlap)
        assert tuple(int(x) for x in sums) == S.np_shift(ta, tb, int(want["dx"][0]), int(want["dy"][0])) and score == want["score"][0]
        if i < 4:
            t = np.asarray(S.VIEWS[i], np.float64)
            print(f"seed {seed} view {i}: shift ({recs[i]['dx']}, {recs[i]['dy']}) for -t / 8 = {-t / 8}, score {recs[i]['score']:.3f}, second {recs[i]['second']:.3f}")
            assert recs[i]["flags"] == _capi.PS_FOUND
            assert abs(recs[i]["dx"] + t[0] / 8) <= 1.0 and abs(recs[i]["dy"] + t[1] / 8) <= 1.0
            assert np.array_equal(recs[i]["start_px"], np.tile(np.array([8.0 * recs[i]["dx"], 8.0 * recs[i]["dy"]], np.float32), 4))
        else:
            print(f"seed {seed} unrelated: score {recs[i]['score']:.3f}")
            assert recs[i]["flags"] == _capi.PS_LOW_SCORE and np.array_equal(recs[i]["start_px"].view(np.uint32), NAN32)


@pytest.mark.parametrize("name", sorted(S.hostile()))
def test_hostile_thumbnails(sref, name):
    """the hand-built thumbnails: the header equals the numpy restatement byte for byte, and the tie order and flags are the expected ones"""
    a, b, o, truth = S.hostile()[name]
    rec, scores = S.ref_search(sref, a, b, o)
    want, table = S.np_search(a, b, o)
    assert np.array_equal(scores.view(np.uint64), table.view(np.uint64))
    _same_record(rec[0], want[0])
    r = rec[0]
    outside = np.ones((S.NSY, S.NSX), bool)
    outside[S.RY - o.radius_y:S.RY + o.radius_y + 1, S.RX - o.radius_x:S.RX + o.radius_x + 1] = False
    assert np.isnan(scores[outside]).all()
    if name == "two-equal-peaks":
        twin = scores[r["dy"] + S.RY, -r["dx"] + S.RX]
        assert r["dx"] < 0 and twin == r["score"]                      # equal score, equal radius, equal dy: the smaller dx
        assert (r["dx2"], r["dy2"]) == (-r["dx"], r["dy"]) and r["second"] == r["score"] and r["flags"] in (_capi.PS_AMBIGUOUS, _capi.PS_LOW_SCORE)
        at = lambda dx, dy: (dy + S.RY) * S.NSX + dx + S.RX                 # noqa: E731
        bt = sref.photo_search_ref_better
        assert bt(1.0, at(-5, 0), 1.0, at(5, 0)) == 1 and bt(1.0, at(5, 0), 1.0, at(-5, 0)) == 0           # then the smaller dx
        assert bt(1.0, at(0, -1), 1.0, at(-1, 0)) == 1 and bt(1.0, at(1, 0), 1.0, at(0, 1)) == 1           # the smaller dy before the smaller dx
        assert bt(1.0, at(0, 1), 1.0, at(-1, -1)) == 1 and bt(0.5, at(0, 0), 1.0, at(30, 20)) == 0         # the radius before both, the score before all
    elif name == "checker":
        assert (r["dx"], r["dy"], r["score"], r["flags"]) == (0, 0, 1.0, _capi.PS_AMBIGUOUS)
        assert (r["dx2"], r["dy2"], r["second"]) == (0, -2, 1.0)       # radius 4: (0, -2) before (0, 2), (-2, 0) and (2, 0)
        assert scores[S.RY, S.RX + 1] == -1.0
    elif name.startswith("constant"):
        assert r["flags"] == _capi.PS_NO_TEXTURE and np.isnan(scores).all() and (r["dx"], r["dy"], r["n_overlap"], r["score"], r["second"]) == (0, 0, 0, -1.0, -1.0)
        assert np.array_equal(r["start_px"].view(np.uint32), NAN32)
    elif name == "radius-0":
        assert (r["dx"], r["dy"], r["flags"], r["second"], r["n_overlap"]) == (0, 0, _capi.PS_FOUND, -1.0, 1120) and (~np.isnan(scores)).sum() == 1
    elif name.startswith("peak"):
        assert (r["dx"], r["dy"]) == truth and r["flags"] == _capi.PS_FOUND and r["n_overlap"] == 80 and abs(r["score"] - 1.0) < 1e-15
        assert np.array_equal(r["start_px"], np.tile(np.array([8.0 * truth[0], 8.0 * truth[1]], np.float32), 4))
    elif name == "min-overlap-excludes-peak":
        assert np.isnan(scores[truth[1] + S.RY, truth[0] + S.RX]) and (r["dx"], r["dy"]) != truth and r["flags"] != _capi.PS_FOUND
        assert r["n_overlap"] >= o.min_overlap


def test_pick_order(sref):
    """the FOUND candidate of the highest score; ties go to the held keyframe (index 0), then the lower slot; a candidate that does not exist or is not
    FOUND is never picked"""
    recs = np.zeros(4, S.SEARCH)
    recs["flags"], recs["score"] = _capi.PS_FOUND, (0.9, 0.95, 0.95, 0.8)
    assert S.ref_pick(sref, recs, [1, 1, 1, 1]) == 1
    assert S.ref_pick(sref, recs, [1, 0, 1, 1]) == 2
    recs["score"] = 0.9
    assert S.ref_pick(sref, recs, [1, 1, 1, 1]) == 0 and S.ref_pick(sref, recs, [0, 1, 1, 1]) == 1
    recs["flags"][:3] = _capi.PS_AMBIGUOUS
    assert S.ref_pick(sref, recs, [1, 1, 1, 1]) == 3 and S.ref_pick(sref, recs, [1, 1, 1, 0]) == -1


def _state(key_px=None):
    s = K.new_state()
    s["has_key"], s["age"], s["keyframes"] = 1, 3, 5
    s["key_px"] = np.arange(8, dtype=np.float32) if key_px is None else key_px
    s["h_origin_key"] = np.array([[1.0, 0, 7.0], [0, 1.0, -3.0], [0, 0, 1.0]])
    return s


def _rec(offsets, flags=0, mse=4.0, n_valid=70000):
    r = np.zeros(1, K.REC)
    r["px"]["offsets_px"], r["px"]["flags"], r["px"]["mse"], r["px"]["n_valid"] = offsets, flags, mse, n_valid
    return r


START = np.tile(np.array([96.0, -56.0], np.float32), 4)
FOUND_AT = (START + np.array([1.5, -2.0, 0.5, 1.0, -1.0, 0.25, 2.0, -0.5], np.float32)).astype(np.float32)
NAN_AT = FOUND_AT.copy()
NAN_AT[5] = np.nan
DECIDE = {
    "retracked": (dict(), _rec(FOUND_AT), _capi.RL_RETRACKED),
    "stopped-singular": (dict(), _rec(FOUND_AT, flags=U.SINGULAR), _capi.RL_STOPPED),
    "stopped-degenerate": (dict(), _rec(FOUND_AT, flags=U.DEGENERATE), _capi.RL_STOPPED),
    "stopped-few-pixels": (dict(), _rec(FOUND_AT, flags=U.FEW_PIXELS), _capi.RL_STOPPED),
    "mse-above-max": (dict(max_mse=3.0), _rec(FOUND_AT), _capi.RL_MSE_ABOVE_MAX),
    "mse-nan": (dict(max_mse=3.0), _rec(FOUND_AT, mse=np.nan), _capi.RL_MSE_ABOVE_MAX),
    "non-finite": (dict(), _rec(NAN_AT), _capi.RL_NON_FINITE),
    "low-overlap": (dict(), _rec(FOUND_AT, n_valid=35839), _capi.RL_LOW_OVERLAP),
    "closure-above-max": (dict(max_closure_px=1.9), _rec(FOUND_AT), _capi.RL_CLOSURE_ABOVE_MAX),
    "closure-at-max": (dict(max_closure_px=2.0), _rec(FOUND_AT), _capi.RL_RETRACKED),
    "stopped-before-mse": (dict(max_mse=3.0, max_closure_px=0.1), _rec(NAN_AT, flags=U.SINGULAR, n_valid=10), _capi.RL_STOPPED),
}


@pytest.mark.parametrize("name", sorted(DECIDE))
def test_decide_relocalise_cases(sref, name):
    """every reason on an input of its own, in decide_revisit's order without CHAIN, and RETRACKED: key_px becomes the record's offsets and nothing else
    of the state changes; h_origin_curr and closure_px against numpy; a rejected call leaves the state byte for byte"""
    kw, rec, want = DECIDE[name]
    s, o = _state(), S.reloc_opts(**kw)
    hb = K.homography(s["key_px"][0]) @ s["h_origin_key"][0]
    hb = hb / hb[2, 2]
    ns, out = S.ref_decide(sref, s, START, hb, rec, o)
    r = out[0]
    assert r["flags"] == want and (r["slot"], r["links"], r["grid"]) == (-1, 0, 0) and not r["pad"].any()
    assert r["rec"].tobytes() == rec[0].tobytes() and np.array_equal(r["start_px"], START) and np.array_equal(r["h_origin_before"], hb)
    assert r["overlap"] == rec["px"]["n_valid"][0] / 71680.0
    if want == _capi.RL_RETRACKED:
        keep = s.copy()
        keep["key_px"] = FOUND_AT
        assert ns.tobytes() == keep.tobytes() and np.array_equal(r["key_px"], FOUND_AT)
        hc = K.homography(FOUND_AT) @ s["h_origin_key"][0]
        hc = hc / hc[2, 2]
        assert np.abs(r["h_origin_curr"] - hc).max() < 1e-9 * np.abs(hc).max()
        assert np.abs(r["closure_px"] - (K.corners(hc) - K.corners(hb))).max() < 1e-8
    else:
        assert ns.tobytes() == s.tobytes() and np.array_equal(r["key_px"], s["key_px"][0])
        assert np.array_equal(r["h_origin_curr"], hb) and not r["closure_px"].any()


def test_rejected_and_candidate_less_calls_change_nothing(sref):
    """a whole relocalise on the host that finds nothing (an unrelated frame) or is rejected (max_closure_px = 1e-3) leaves the state, the keyframe, the
    map state, the entries and the images byte for byte, with and without a map; the record says why"""
    seed = 1
    frames, _, _ = S.kidnapped(seed)
    _, _, _, other = S.cases(seed)
    for capacity in (0, S.CAPACITY):
        ses = S.RefRelocSession(sref, capacity)
        to = K.opts(**S.KIDNAP_TRACK)
        ses.track(frames[0], None, to)
        ses.track(frames[1], None, to)
        before = ses.snapshot()
        none = ses.relocalise(other, S.reloc_opts())
        assert none["rv"]["flags"] == _capi.RL_NO_CANDIDATE and none["target"] == _capi.RL_TARGET_NONE and none["n_found"] == 0 and none["n_searched"] >= 1
        assert not none["rv"]["rec"].tobytes().strip(b"\0") and not none["search"].tobytes().strip(b"\0")
        assert np.array_equal(none["rv"]["start_px"].view(np.uint32), NAN32) and ses.snapshot() == before
        rej = ses.relocalise(frames[1], S.reloc_opts(max_closure_px=1e-3))
        assert rej["rv"]["flags"] == _capi.RL_CLOSURE_ABOVE_MAX and rej["target"] == _capi.RL_TARGET_HELD and rej["search"]["flags"] == _capi.PS_FOUND
        assert ses.snapshot() == before


def test_kidnapped_rows(sref):
    """the host reference on the two kidnapped rows over seeds 1, 2, 5, 11.  Kidnapped: the track from a zero step at 4 levels ends far from the truth, the
    relocalise on the same frame is RETRACKED on the held keyframe, the next track with the true step is TRACKED.  Kidnapped with a map: after the
    bridged re-key on a constant frame the chain is far off; the relocalise attaches slot 0.  The gates of photo_search_util are twice the worst error
    printed here."""
    worst, worst_map = 0.0, 0.0
    for seed in S.SEEDS:
        ses = S.RefRelocSession(sref, 0)
        lost, rl, nxt = S.run_kidnapped(seed, ses.track, ses.relocalise)
        _, poses, _ = S.kidnapped(seed)
        e_lost, e_rl, e_next = S.worst_px(lost["key_px"], poses[1]), S.worst_px(rl["rv"]["key_px"], poses[1]), S.worst_px(nxt["key_px"], poses[2])
        print(f"kidnapped, seed {seed}: track flags {lost['flags']} at {e_lost:.2f} px; search ({rl['search']['dx']}, {rl['search']['dy']}) score "
              f"{rl['search']['score']:.3f}; relocalise flags {rl['rv']['flags']} at {e_rl:.4f} px; next track flags {nxt['flags']} at {e_next:.4f} px")
        assert (lost["flags"] & _capi.KF_LOST) or e_lost > S.BEFORE_RATIO * S.GATE_KIDNAPPED
        assert rl["rv"]["flags"] == _capi.RL_RETRACKED and rl["target"] == _capi.RL_TARGET_HELD and not (nxt["flags"] & _capi.KF_LOST)
        assert np.array_equal(ses.state["key_px"][0], nxt["key_px"])
        worst = max(worst, e_rl)
        ses = S.RefRelocSession(sref, S.CAPACITY)
        far, rm = S.run_kidnapped_map(seed, ses.track, ses.relocalise)
        _, _, pose = S.kidnapped_map(seed)
        e_before, e_after = KM.worst_px(rm["rv"]["h_origin_before"], pose), KM.worst_px(rm["rv"]["h_origin_curr"], pose)
        print(f"kidnapped with a map, seed {seed}: track flags {far['flags']}; searched {rm['n_searched']}, found {rm['n_found']}, target {rm['target']}, "
              f"score {rm['search']['score']:.3f}; h_origin_curr {e_before:.3f} px -> {e_after:.4f} px")
        assert far["flags"] & _capi.KF_LOST and rm["rv"]["flags"] == _capi.RL_ATTACHED and rm["target"] == 0 and rm["rv"]["slot"] == 0
        assert e_before >= S.BEFORE_RATIO * S.GATE_KIDNAPPED_MAP
        assert ses.mstate["cur_slot"][0] == 0 and np.array_equal(ses.state["h_origin_key"][0], ses.entries["h_origin_key"][0])
        worst_map = max(worst_map, e_after)
    print(f"worst after the relocalise: kidnapped {worst:.4f} px, with a map {worst_map:.4f} px")
    assert worst <= S.GATE_KIDNAPPED / 2 and worst_map <= S.GATE_KIDNAPPED_MAP / 2
    assert worst > 0.9 * S.GATE_KIDNAPPED / 2 and worst_map > 0.9 * S.GATE_KIDNAPPED_MAP / 2        # the gates are these measurements, not wider


def test_photo_search_check_under_asan_ubsan(tmp_path):
    """the reference core, every shift of the range on heap thumbnails, the hostile thumbnails and two relocalises under AddressSanitizer + UBSan: a
    stand-alone program; nothing loaded into python is sanitized"""
    exe = str(tmp_path / "photo_search_check_san.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *U.HOST_FLAGS,
                    os.path.join(ROOT, "tests", "cpp", "photo_search_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "photo_search_check: ok" in r.stdout
