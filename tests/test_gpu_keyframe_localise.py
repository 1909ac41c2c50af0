"""hnet_op_keyframe_localise on the device (include/hnet.h; csrc/kernels_keyframe_localise.hip, capi_keyframe_localise.hip): template and cover
against hnet_op_keyframe_render, rec against hnet_op_photo_align_masked, the whole record against the host header run on the device's alignment record (7q's
method), the composite rows within their CPU-fixed gates, the verdicts an input can reach, m = 1 and 8 with an invalid and a singular entry, and the
refusals.  Main model prior-3, N = 16, max_batch 8."""
import ctypes as C

import numpy as np
import pytest

import keyframe_localise_util as KL
import keyframe_render_util as KR
import keyframe_util as K
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

INVALID = 1


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return KL.build_rule_ref(tmp_path_factory.mktemp("keyframe_localise_ref_gpu"))


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=8)
    yield e
    e.close()


def _check_identities(eng, lib, images, entries, view, frame, mode=_capi.RENDER_FEWEST_LINKS, **kw):
    """one localise call -> its record; asserted on the way: template and cover = hnet_op_keyframe_render's, rec = hnet_op_photo_align_masked's on them (zeros
    when nothing was aligned), the whole record = the host header's decide_localise on the device's alignment record"""
    out, tmpl, cover = eng.op_keyframe_localise(images, entries, view, frame, want_images=True, mode=mode, **kw)
    assert eng.op_keyframe_localise(images, entries, view, frame, mode=mode, **kw).tobytes() == out.tobytes()      # (without the images: the same record)
    rimg, rcover, rrec = eng.op_keyframe_render(images, entries, view, 320, 224, mode)
    assert tmpl.tobytes() == rimg.tobytes() and cover.tobytes() == rcover.tobytes()
    r = out[0]
    assert r["used_mask"] == rrec[0]["used_mask"] and r["cover"] == int(rrec[0]["n_covered"]) / 71680.0
    akw = {k: v for k, v in kw.items() if k in ("max_iterations", "min_valid", "lambda0", "eps_px", "brightness", "huber_k", "gain0", "bias0")}
    akw.setdefault("max_iterations", 6)
    levels = kw.get("levels", 3)
    o = KL.loc_opts(mode=mode, **kw)
    if r["flags"] in (_capi.LOC_NO_MAP, _capi.LOC_LOW_COVER):
        assert not r["rec"].tobytes().strip(b"\0")
        arec = np.zeros(1, _capi.PHOTO_ROBUST_DTYPE)
    else:
        arec = eng.op_photo_align_masked(tmpl, cover, frame, np.zeros(8, np.float32), levels=levels, **akw)
        assert r["rec"].tobytes() == arec[0].tobytes()
    _, want, _, _, _ = KL.ref_decide(lib, None, None, entries, int(rrec[0]["used_mask"]), int(rrec[0]["n_covered"]), view, arec, o)
    assert out.tobytes() == want.tobytes(), (int(r["flags"]), int(want[0]["flags"]))
    return r


@pytest.mark.parametrize("name", list(KL.ROWS))
def test_composite_rows_localise(eng, lib, name):
    """the composite rows on seeds 1, 2, 5, 11 (scenes on which the revisit's select has no candidate: tests/test_photo_masked_cpu.py): LOCALISED, the offsets
    within the row's gate of the truth, the corners of h_origin_curr within the gate of the camera's true pose (printed beside the prediction's error), and
    the three identities"""
    gate = KL.GATES[name]
    for seed in KL.SEEDS:
        s = KL.scene(name, seed)
        r = _check_identities(eng, lib, s["images"], s["entries"], s["view"], s["frame"])
        err = KL.worst_corner_px(r["rec"]["px"]["offsets_px"], s["truth"])
        before, after = np.abs(K.corners(s["view"]) - s["cam_pose"]).max(), np.abs(K.corners(r["h_origin_curr"]) - s["cam_pose"]).max()
        print(f"{name} seed {seed}: flags {r['flags']}, cover {r['cover']:.3f}, overlap {r['overlap']:.3f}, offsets {err:.4f} px from the truth (gate {gate:.4f}), "
              f"pose {before:.3f} -> {after:.4f} px, correction up to {np.abs(r['correction_px']).max():.3f} px")
        assert r["flags"] == _capi.LOC_LOCALISED and r["links"] == 1 + int(s["entries"]["links"].max()) and r["links_before"] == 0
        assert err < gate and after < gate, (name, seed, err, after)


def test_verdicts_an_input_reaches(eng, lib):
    """NO_MAP (no valid entry), LOW_COVER (min_cover above the composite's 0.75), STOPPED (min_valid above the mask's pixels: FEW_PIXELS), MSE_ABOVE_MAX,
    LOW_OVERLAP, SHIFT_ABOVE_MAX and LOCALISED on the two-keyframe scene, each with the three identities; a rejected call states no correction.  (NON_FINITE
    and CHAIN need a record no image produces: tests/test_keyframe_localise_cpu.py.)"""
    s = KL.scene("two-keyframes-drift8", 2)
    none = s["entries"].copy()
    none["valid"] = 0
    cases = [(_capi.LOC_NO_MAP, none, {}), (_capi.LOC_LOW_COVER, s["entries"], dict(min_cover=0.9)), (_capi.LOC_STOPPED, s["entries"], dict(min_valid=60000)),
             (_capi.LOC_MSE_ABOVE_MAX, s["entries"], dict(max_mse=0.01)), (_capi.LOC_LOW_OVERLAP, s["entries"], dict(min_overlap=0.9)),
             (_capi.LOC_SHIFT_ABOVE_MAX, s["entries"], dict(max_shift_px=1.0)), (_capi.LOC_LOCALISED, s["entries"], dict(max_mse=5.0, max_shift_px=20.0))]
    for flag, ent, kw in cases:
        r = _check_identities(eng, lib, s["images"], ent, s["view"], s["frame"], **kw)
        assert r["flags"] == flag, (flag, int(r["flags"]), kw)
        if flag != _capi.LOC_LOCALISED:
            assert not r["correction_px"].any() and r["h_origin_curr"].tobytes() == r["h_origin_before"].tobytes()


def test_one_entry_and_eight_with_an_invalid_and_a_singular_one(eng, lib):
    """m = 1: one keyframe 200 px away covers 0.37 of the view: LOW_COVER by default, LOCALISED with min_cover and min_overlap at 0.2.  m = 8: the scene's two
    entries among an invalid one, one whose h_origin_key is singular (the render skips both) and four more copies with more links, in MEAN mode too: the
    identities hold and the record equals the host's"""
    s = KL.scene("two-keyframes-drift8", 5)
    r = _check_identities(eng, lib, s["images"][:1], s["entries"][:1], s["view"], s["frame"])
    assert r["flags"] == _capi.LOC_LOW_COVER and r["used_mask"] == 1 and 0.3 < r["cover"] < 0.45
    r = _check_identities(eng, lib, s["images"][:1], s["entries"][:1], s["view"], s["frame"], min_cover=0.2, min_overlap=0.2, min_valid=5000)
    print(f"m = 1: flags {r['flags']}, cover {r['cover']:.3f}, overlap {r['overlap']:.3f}, offsets {KL.worst_corner_px(r['rec']['px']['offsets_px'], s['truth']):.4f} px off")
    assert r["flags"] == _capi.LOC_LOCALISED and r["links"] == 2
    pick = [0, 1, 0, 1, 0, 1, 0, 1]
    images, ent = s["images"][pick], s["entries"][pick].copy()
    ent["links"] = [4, 5, 0, 0, 1, 2, 6, 7]
    ent["serial"] = np.arange(1, 9)
    ent[2]["valid"] = 0
    ent[3]["h_origin_key"] = 0.0
    for mode in (_capi.RENDER_FEWEST_LINKS, _capi.RENDER_MEAN):
        r = _check_identities(eng, lib, images, ent, s["view"], s["frame"], mode=mode)
        assert r["used_mask"] == 0b11110011 and r["flags"] == _capi.LOC_LOCALISED and r["links"] == 8
        assert KL.worst_corner_px(r["rec"]["px"]["offsets_px"], s["truth"]) < KL.GATES["two-keyframes-drift8"]


def test_refusals_write_nothing(eng):
    """a null argument but the last two, m outside 1 .. 8, refused options and a non-finite view return HNET_ERR_INVALID_ARG and leave out, out_template and
    out_cover untouched"""
    L = _capi.lib()
    s = KL.scene("two-keyframes-drift8", 1)
    img, ent, view, cur = np.ascontiguousarray(s["images"]), np.ascontiguousarray(s["entries"]), np.ascontiguousarray(s["view"]), np.ascontiguousarray(s["frame"])
    out, tmpl, cover = np.full(_capi.KEYFRAME_LOCALISE_DTYPE.itemsize, 0xA5, np.uint8), np.full(71680, 0x5A, np.uint8), np.full(71680, 0x3C, np.uint8)
    ok = _capi.keyframe_localise_opts()

    def call(m=2, images=img.ctypes.data, entries=ent.ctypes.data, v=view, curr=cur.ctypes.data, o=ok, outp=out.ctypes.data):
        return L.hnet_op_keyframe_localise(eng.handle, m, images, entries, None if v is None else v.ctypes.data, curr, None if o is None else C.addressof(o), outp,
                                           tmpl.ctypes.data, cover.ctypes.data)
    assert call(images=None) == INVALID and call(entries=None) == INVALID and call(v=None) == INVALID and call(curr=None) == INVALID and call(o=None) == INVALID
    assert call(outp=None) == INVALID and call(m=0) == INVALID and call(m=9) == INVALID and call(m=-1) == INVALID
    bad_view = view.copy()
    bad_view[1, 2] = np.inf
    assert call(v=bad_view) == INVALID
    nan = float("nan")
    for kw in (dict(levels=0), dict(levels=5), dict(mode=3), dict(min_cover=1.5), dict(min_cover=nan), dict(min_overlap=-0.1), dict(max_mse=-1.0), dict(max_shift_px=nan),
               dict(apply=2), dict(huber_k=-1.0), dict(max_iterations=33), dict(brightness=0, gain0=2.0)):
        assert call(o=_capi.keyframe_localise_opts(**kw)) == INVALID, kw
    assert (out == 0xA5).all() and (tmpl == 0x5A).all() and (cover == 0x3C).all()
    assert call() == 0 and not (out == 0xA5).all() and not (tmpl == 0x5A).all()
