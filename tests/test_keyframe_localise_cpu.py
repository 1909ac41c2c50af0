"""The localise rule (include/hnet_keyframe_localise.h; include/hnet.h hnet_op_keyframe_localise) on the CPU, through
tests/cpp/keyframe_localise_ref.cpp: the eligible entries, the start, every verdict of decide_localise on an input of its own and in the header's order,
the record of a localised call against numpy, and apply (the held keyframe's new place, the links rule, the invariant with cur_slot, and no byte changed
otherwise).  The template and the alignment record come from the host references of the render and of the masked alignment."""
import numpy as np
import pytest

import keyframe_localise_util as KL
import keyframe_map_util as KM
import keyframe_render_util as KR
import keyframe_util as K
import photo_align_util as U
import photo_masked_util as M
from cuahn_vio_amd import _capi

NAME, SEED = "two-keyframes-drift8", 1
APPLY_BOUND_PX = 1e-9          # origin_curr of the applied state against h_origin_curr: one inverse and two products in double


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return KL.build_rule_ref(tmp_path_factory.mktemp("keyframe_localise_ref"))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the two-keyframe scene of seed 1: (scene, render record, level-0 record of the masked reference from zero offsets)"""
    tmp = tmp_path_factory.mktemp("keyframe_localise_case")
    s = KL.scene(NAME, SEED)
    comp, cover, rrec = KL.composite(KR.build_ref(tmp), NAME, SEED)
    rec = M.ref_run(M.build_ref(tmp), comp, cover, s["frame"], np.zeros(8, np.float32), KL.LEVELS, max_iterations=KL.TRIALS)[0]
    return s, rrec, rec


def test_defaults_and_refused_options(lib):
    """the defaults (choices, not measurements) and what opts_valid refuses"""
    import ctypes as C
    o = _capi.KeyframeLocaliseOpts()
    lib.keyframe_localise_ref_default_opts(C.byref(o))
    assert bytes(o) == bytes(KL.loc_opts(max_iterations=6)) and (o.levels, o.mode, o.min_cover, o.min_overlap, o.max_mse, o.max_shift_px, o.apply) == (3, 0, 0.5, 0.4, 0.0, 0.0, 0)
    ok = lambda **kw: lib.keyframe_localise_ref_opts_valid(C.byref(KL.loc_opts(**kw)))
    assert ok() and ok(apply=1, mode=2, levels=4, min_cover=0.0, min_overlap=1.0, max_mse=5.0, max_shift_px=20.0)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(levels=0), dict(levels=5), dict(mode=3), dict(mode=-1), dict(min_cover=-0.1), dict(min_cover=1.1), dict(min_cover=nan), dict(min_overlap=1.5),
               dict(min_overlap=nan), dict(max_mse=-1.0), dict(max_mse=inf), dict(max_shift_px=-1.0), dict(max_shift_px=nan), dict(apply=2), dict(apply=-1),
               dict(huber_k=-1.0), dict(max_iterations=33)):
        assert not ok(**kw), kw


def test_eligible_and_start(lib):
    """select's preference: valid, not the current slot, strictly fewer links than the chain; without a map state every valid entry.  The start is zeros,
    or quiet NaNs when no entry took part or the cover is below min_cover"""
    e = KR.entries([np.eye(3)] * 5, links=[0, 3, 5, 2, 9], valid=[1, 1, 1, 0, 1])
    m = np.zeros(1, KM.MSTATE)
    m["cur_slot"], m["cur_links"] = 1, 5
    assert KL.ref_eligible_mask(lib, m, e) == 0b00001            # slot 1 is held, 2 has as many links, 3 is invalid, 4 has more
    m["cur_slot"], m["cur_links"] = -1, 10
    assert KL.ref_eligible_mask(lib, m, e) == 0b10111
    assert KL.ref_eligible_mask(lib, None, e) == 0b10111
    o = KL.loc_opts()
    assert not KL.ref_start(lib, 3, 35840, o).any() and KL.ref_start(lib, 3, 35840, o).tobytes() == np.zeros(8, np.float32).tobytes()      # exactly min_cover
    for used, n in ((0, 71680), (3, 35839), (3, 0)):
        assert (KL.ref_start(lib, used, n, o).view(np.uint32) == 0x7FC00000).all(), (used, n)


def test_every_verdict_in_order(lib, case):
    """all faults at once give NO_MAP; taking them away one by one in the header's order gives LOW_COVER, STOPPED, MSE_ABOVE_MAX, NON_FINITE, LOW_OVERLAP,
    SHIFT_ABOVE_MAX, CHAIN and LOCALISED.  A rejected call leaves h_origin_curr = h_origin_before, a zero correction and links = links_before; cover and
    used_mask are reported always, overlap only when something was aligned"""
    s, rrec, rec = case
    n_cov, line = int(rrec["n_covered"][0]), np.array([0, 0, 10, 5, 20, 10, 30, 15], np.float32) - np.array([0, 0, 0, 223, 319, 223, 319, 0], np.float32)
    bad = rec.copy()
    bad["px"]["flags"] |= U.FEW_PIXELS
    bad["px"]["offsets_px"][0, 3] = np.nan
    faults = dict(used_mask=0, n_covered=1000, rec=bad, o=dict(max_mse=0.01, min_overlap=0.9, max_shift_px=1.0))
    want = [_capi.LOC_NO_MAP, _capi.LOC_LOW_COVER, _capi.LOC_STOPPED, _capi.LOC_MSE_ABOVE_MAX, _capi.LOC_NON_FINITE, _capi.LOC_LOW_OVERLAP, _capi.LOC_SHIFT_ABOVE_MAX,
            _capi.LOC_CHAIN, _capi.LOC_LOCALISED]
    got = []
    for step in range(9):
        if step == 1: faults["used_mask"] = 3
        if step == 2: faults["n_covered"] = n_cov
        if step == 3: faults["rec"] = faults["rec"].copy(); faults["rec"]["px"]["flags"] &= ~U.FEW_PIXELS
        if step == 4: faults["o"].pop("max_mse")
        if step == 5: faults["rec"] = faults["rec"].copy(); faults["rec"]["px"]["offsets_px"][0] = line      # finite, but four corners on one line
        if step == 6: faults["o"].pop("min_overlap")
        if step == 7: faults["o"].pop("max_shift_px")
        if step == 8: faults["rec"] = rec
        loc, out, _, _, _ = KL.ref_decide(lib, None, None, s["entries"], faults["used_mask"], faults["n_covered"], s["view"], faults["rec"], KL.loc_opts(**faults["o"]))
        r = out[0]
        got.append(int(r["flags"]))
        assert loc == (r["flags"] == _capi.LOC_LOCALISED) and r["used_mask"] == faults["used_mask"] and r["cover"] == faults["n_covered"] / 71680.0
        assert r["links_before"] == 0 and not r["pad"].any() and r["h_origin_before"].tobytes() == np.ascontiguousarray(s["view"]).tobytes()
        assert r["overlap"] == (0.0 if step < 2 else int(faults["rec"]["px"]["n_valid"][0]) / 71680.0)
        if not loc:
            assert r["h_origin_curr"].tobytes() == r["h_origin_before"].tobytes() and not r["correction_px"].any() and r["links"] == 0
    assert got == want, got


def test_localised_record_against_numpy(lib, case):
    """h_origin_curr = H(offsets) . h_origin_before (numpy, normalised), correction_px the corners' difference, links = 1 + the largest links of the
    entries that took part; the pose it states lies within the row's gate of the camera's true pose where the prediction was 6 px off"""
    s, rrec, rec = case
    loc, out, _, _, _ = KL.ref_decide(lib, None, None, s["entries"], 3, int(rrec["n_covered"][0]), s["view"], rec, KL.loc_opts())
    r = out[0]
    assert loc == 1 and r["flags"] == _capi.LOC_LOCALISED and r["links"] == 1 + int(s["entries"]["links"].max()) and r["rec"].tobytes() == rec[0].tobytes()
    h = K.homography(rec[0]["px"]["offsets_px"].astype(np.float64)) @ s["view"]
    h = h / h[2, 2]
    assert np.abs(K.corners(r["h_origin_curr"]) - K.corners(h)).max() < 1e-9
    assert np.abs(r["correction_px"] - (K.corners(r["h_origin_curr"]) - K.corners(s["view"]))).max() < 1e-9
    before, after = np.abs(K.corners(s["view"]) - s["cam_pose"]).max(), np.abs(K.corners(r["h_origin_curr"]) - s["cam_pose"]).max()
    print(f"pose error before {before:.3f} px, after {after:.4f} px (gate {KL.GATES[NAME]:.4f})")
    assert after < KL.GATES[NAME] and before >= KL.BEFORE_GATES * KL.GATES[NAME]


def _session(s, cur_slot):
    """a session whose chain predicts s's view: key_px a 5 px warp, h_origin_key = inverse(H(key_px)) . view; the map holds the scene's two entries and, in
    slot 2, the held keyframe with 7 links (cur_slot = 2) or nothing of it (cur_slot = -1)"""
    key = K.homography(np.zeros(8)).astype(np.float64)
    key_px = (np.arange(8) - 3.5).astype(np.float32)
    hk = np.linalg.inv(K.homography(key_px.astype(np.float64))) @ s["view"]
    hk = hk / hk[2, 2]
    st = np.zeros(1, K.STATE)
    st["has_key"], st["age"], st["keyframes"], st["key_px"], st["h_origin_key"] = 1, 4, 9, key_px, hk
    e = np.zeros(3, KR.ENTRY)
    e[:2] = s["entries"]
    e[2]["valid"], e[2]["links"], e[2]["serial"], e[2]["h_origin_key"] = 1, 7, 9, hk
    m = np.zeros(1, KM.MSTATE)
    m["cur_slot"], m["cur_links"], m["cursor"], m["serial"] = cur_slot, 7, 1, 9
    del key
    return st, m, e


@pytest.mark.parametrize("cur_slot", [2, -1])
def test_apply(lib, case, cur_slot):
    """apply = 1 on a localised call: key_px, age, keyframes, cursor and serial stay; origin_curr of the new state lies within 1e-9 px of h_origin_curr (printed);
    cur_links and the held entry's links become 1 + the largest links that took part, never more than before; the entry of cur_slot carries the state's new
    h_origin_key byte for byte (none when cur_slot = -1); the other entries keep every byte.  apply = 0 and a rejected call change no byte of any state"""
    s, rrec, rec = case
    st, m, e = _session(s, cur_slot)
    used = KL.ref_eligible_mask(lib, m, e)
    assert used == 0b011
    n_cov = int(rrec["n_covered"][0])
    loc, out, ns, nm, ne = KL.ref_decide(lib, st, m, e, used, n_cov, s["view"], rec, KL.loc_opts(apply=1))
    r = out[0]
    assert loc == 1 and r["links_before"] == 7 and r["links"] == 3
    assert ns["key_px"].tobytes() == st["key_px"].tobytes() and (ns["has_key"], ns["age"], ns["keyframes"]) == (st["has_key"], st["age"], st["keyframes"])
    new_curr = K.homography(ns[0]["key_px"].astype(np.float64)) @ ns[0]["h_origin_key"]
    d = float(np.abs(K.corners(new_curr / new_curr[2, 2]) - K.corners(r["h_origin_curr"])).max())
    print(f"cur_slot {cur_slot}: origin_curr of the applied state against h_origin_curr: {d:.3e} px (bound {APPLY_BOUND_PX:.0e})")
    assert d < APPLY_BOUND_PX
    assert nm["cur_links"] == 3 <= m["cur_links"] and (nm["cur_slot"], nm["cursor"], nm["serial"]) == (m["cur_slot"], m["cursor"], m["serial"])
    assert ne[:2].tobytes() == e[:2].tobytes()
    if cur_slot >= 0:
        assert ne[2]["h_origin_key"].tobytes() == ns[0]["h_origin_key"].tobytes() and ne[2]["links"] == 3 and (ne[2]["valid"], ne[2]["serial"]) == (1, 9)
    else:
        assert ne[2].tobytes() == e[2].tobytes()
    for o, rr in ((KL.loc_opts(apply=0), rec), (KL.loc_opts(apply=1, max_shift_px=1.0), rec), (KL.loc_opts(apply=1, max_mse=0.01), rec)):
        loc2, out2, ns2, nm2, ne2 = KL.ref_decide(lib, st, m, e, used, n_cov, s["view"], rr, o)
        assert ns2.tobytes() == st.tobytes() and nm2.tobytes() == m.tobytes() and ne2.tobytes() == e.tobytes()
        assert out2[0]["links_before"] == 7 and out2[0]["links"] == (3 if loc2 else 7)
    # a held keyframe whose key_px has no homography: the new place cannot be formed, the verdict is CHAIN and nothing changes
    st_bad = st.copy()
    st_bad["key_px"][0] = np.array([0, 0, 10, 5, 20, 10, 30, 15], np.float32) - np.array([0, 0, 0, 223, 319, 223, 319, 0], np.float32)
    loc3, out3, ns3, nm3, ne3 = KL.ref_decide(lib, st_bad, m, e, used, n_cov, s["view"], rec, KL.loc_opts(apply=1))
    assert loc3 == 0 and out3[0]["flags"] == _capi.LOC_CHAIN and ns3.tobytes() == st_bad.tobytes() and nm3.tobytes() == m.tobytes() and ne3.tobytes() == e.tobytes()
    assert not out3[0]["correction_px"].any() and out3[0]["h_origin_curr"].tobytes() == out3[0]["h_origin_before"].tobytes()
