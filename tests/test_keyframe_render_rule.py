"""The rule of the keyframe render on the host (include/hnet_keyframe_render.h, tests/cpp/keyframe_render_ref.cpp), no GPU: render_setup,
render_sample at the edges of its domain, the three modes of render_pixel on hand-made pixels, the counter identities of a whole render, render_fit_view,
and the ranks of the texture map that the GPU test relies on."""
import ctypes as C

import numpy as np
import pytest

import keyframe_render_util as R
import keyframe_util as K
from cuahn_vio_amd import _capi, synth

FEW, NEW, MEAN = R.MODES


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return R.build_ref(tmp_path_factory.mktemp("keyframe_render_ref"))


def _ramp():
    """img[y][x] = (7 x + 13 y) % 256: every byte tells where it was read"""
    y, x = np.mgrid[0:R.H, 0:R.W]
    return ((7 * x + 13 * y) % 256).astype(np.uint8)


def test_layouts_and_symbols(rref):
    header = open(K.ROOT + "/include/hnet.h").read()
    for name in ("hnet_keyframe_render_fit_view", "hnet_op_keyframe_render", "hnet_sessions_enable_keyframe_render", "hnet_sessions_keyframe_render"):
        assert name in _capi.SYMBOLS and name in header
    assert (_capi.RENDER_FEWEST_LINKS, _capi.RENDER_NEWEST, _capi.RENDER_MEAN) == (0, 1, 2) and R.REC.itemsize == 224
    for w, h, mode, ok in ((1, 1, 0, 1), (8192, 8192, 2, 1), (0, 5, 0, 0), (5, 0, 0, 0), (8193, 5, 0, 0), (5, 8193, 0, 0), (5, 5, 3, 0), (5, 5, -1, 0)):
        assert rref.keyframe_render_ref_opts_valid(C.byref(_capi.KeyframeRenderOpts(w, h, mode, 0))) == ok, (w, h, mode)


def test_setup(rref):
    """an identity view gives the entry's h_origin_key bit for bit; a general one h_origin_key . inverse(view) to double rounding; a singular view, an
    invalid entry and non-finite matrices fail"""
    for seed in range(10):
        h = K.homography(synth.true_offsets(seed, 30.0))
        e = R.entries([h])
        s = R.ref_setup(rref, np.eye(3), e)
        assert s is not None and s.tobytes() == h.tobytes()
        view = K.homography(synth.true_offsets(seed + 50, 20.0)) @ np.diag([0.5, 0.5, 1.0])
        s = R.ref_setup(rref, view, e)
        want = h @ np.linalg.inv(view)
        want /= want[2, 2]
        assert s is not None and np.abs(s - want).max() <= 1e-12 * np.abs(want).max()
    e = R.entries([np.eye(3)])
    assert R.ref_setup(rref, np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]]), e) is None           # singular view
    assert R.ref_setup(rref, np.zeros((3, 3)), e) is None
    assert R.ref_setup(rref, np.eye(3), R.entries([np.eye(3)], valid=[0])) is None                              # invalid entry
    bad = np.eye(3)
    bad[0, 1] = np.nan
    assert R.ref_setup(rref, np.eye(3), R.entries([bad])) is None and R.ref_setup(rref, bad, e) is None
    bad[0, 1] = np.inf
    assert R.ref_setup(rref, np.eye(3), R.entries([bad])) is None and R.ref_setup(rref, bad, e) is None
    assert R.ref_setup(rref, np.eye(3), R.entries([np.diag([1.0, 1.0, 0.0])])) is None                          # a product without h[8]


def test_sample_edges(rref):
    img = _ramp()
    eye = np.eye(3)
    for u, v in ((0, 0), (17, 5), (319, 0), (0, 223), (319, 223), (200, 100)):
        assert R.ref_sample(rref, eye, img, u, v) == int(img[v, u])                      # integer positions return the byte
    # x = 319 and y = 223 exactly are valid and the clamped second tap has weight zero: the byte itself, also from a fractional row / column
    assert R.ref_sample(rref, R.shift(319.0, 0.0), img, 0, 7) == int(img[7, 319])
    assert R.ref_sample(rref, R.shift(0.0, 223.0), img, 9, 0) == int(img[223, 9])
    got = R.ref_sample(rref, R.shift(319.0, 0.5), img, 0, 10)
    assert got == int(np.floor(np.float32(0.5) * (np.float32(img[11, 319]) - np.float32(img[10, 319])) + np.float32(img[10, 319]) + np.float32(0.5)))
    # just outside, and behind the camera
    assert R.ref_sample(rref, R.shift(319.0000001, 0.0), img, 0, 0) is None
    assert R.ref_sample(rref, R.shift(0.0, 223.0000001), img, 0, 0) is None
    assert R.ref_sample(rref, R.shift(-1e-9, 0.0), img, 0, 0) is None
    assert R.ref_sample(rref, R.shift(0.0, -1e-9), img, 0, 0) is None
    assert R.ref_sample(rref, np.diag([-1.0, -1.0, -1.0]), img, 5, 5) is None             # z < 0 although x / z is inside
    assert R.ref_sample(rref, np.diag([1.0, 1.0, 0.0]), img, 5, 5) is None                # z = 0
    assert R.ref_sample(rref, np.full((3, 3), np.nan), img, 5, 5) is None
    # a fractional position: the blend in float in the header's order
    s = R.shift(10.25, 20.75)
    a00, a01, a10, a11 = (np.float32(img[20, 10]), np.float32(img[20, 11]), np.float32(img[21, 10]), np.float32(img[21, 11]))
    fx, fy = np.float32(0.25), np.float32(0.75)
    top, bot = a00 + fx * (a01 - a00), a10 + fx * (a11 - a10)
    assert R.ref_sample(rref, s, img, 0, 0) == int(np.floor(top + fy * (bot - top) + np.float32(0.5)))


def test_pixel_modes(rref):
    """a hand-made pixel of three entries: samples 10, 50, 91, links 2, 1, 1, serials 5, 9, 9"""
    vals, links, serials = [10, 50, 91], [2, 1, 1], [5, 9, 9]
    # all three cover: fewest links ties between slots 1 and 2 -> the lower slot; newest ties the same way; mean (151 + 1) / 3 = 50
    for mode, want in ((FEW, 50), (NEW, 50), (MEAN, 50)):
        out, cover, n, sse = R.ref_pixel(rref, vals, 0b111, links, serials, mode)
        assert (out, cover) == (want, 3)
        assert n[:3].tolist() == [1, 1, 1] and sse[:3].tolist() == [40 * 40, 0, 41 * 41] and not n[3:].any() and not sse[3:].any()
    # slots 0 and 2 cover: fewest links -> slot 2 (1 < 2); newest -> slot 2 (9 > 5); mean (101 + 1) / 2 = 51
    for mode, want in ((FEW, 91), (NEW, 91), (MEAN, 51)):
        out, cover, n, sse = R.ref_pixel(rref, vals, 0b101, links, serials, mode)
        assert (out, cover) == (want, 2)
        assert n[:3].tolist() == [1, 0, 1] and sse[:3].tolist() == [(10 - want) ** 2, 0, (91 - want) ** 2]
    # the two modes apart: links prefer slot 0, serials slot 1
    assert R.ref_pixel(rref, [10, 50], 0b11, [0, 3], [1, 2], FEW)[0] == 10
    assert R.ref_pixel(rref, [10, 50], 0b11, [0, 3], [1, 2], NEW)[0] == 50
    # the mean rounds half up: (10 + 11 + 1) / 2 = 11
    assert R.ref_pixel(rref, [10, 11], 0b11, [0, 0], [1, 2], MEAN)[0] == 11
    # one cover: the sample in every mode, no seam statistics; none: 0
    for mode in R.MODES:
        out, cover, n, sse = R.ref_pixel(rref, vals, 0b010, links, serials, mode)
        assert (out, cover) == (50, 1) and not n.any() and not sse.any()
        out, cover, n, sse = R.ref_pixel(rref, vals, 0, links, serials, mode)
        assert (out, cover) == (0, 0) and not n.any() and not sse.any()
    # eight entries, all 255: the sums hold
    out, cover, n, sse = R.ref_pixel(rref, [255] * 8, 0xFF, range(8), range(8), MEAN)
    assert (out, cover) == (255, 8) and n.tolist() == [1] * 8 and not sse.any()


@pytest.mark.parametrize("size", R.VIEWS)
def test_counter_identities(rref, size):
    w, h = size
    images, ent = R.pose_map(3)
    for mode in R.MODES:
        out, cover, rec = R.ref_render(rref, images, ent, R.view(w, h), w, h, mode)
        r = rec[0]
        assert r["h_origin_view"].tobytes() == R.view(w, h).tobytes() and (r["used_mask"], r["skipped_mask"]) == (7, 0)
        assert r["n_covered"] == (cover >= 1).sum() and r["n_overlap"] == (cover >= 2).sum() and r["n_overlap"] <= r["n_covered"] <= w * h
        assert (r["n"] <= r["n_overlap"]).all() and not r["n"][3:].any() and not r["sse"][3:].any() and cover.max() <= 3
        assert not out[cover == 0].any()
        if (w, h) == (320, 224):
            assert r["n_overlap"] > 10000                      # the case does overlap
    # all covering samples equal: no disagreement
    flat = np.full((3, R.H, R.W), 77, np.uint8)
    for mode in R.MODES:
        out, cover, rec = R.ref_render(rref, flat, ent, R.view(w, h), w, h, mode)
        assert not rec[0]["sse"].any() and (out[cover >= 1] == 77).all()


def test_skipped_entries(rref):
    """an invalid entry in the middle and a singular h_origin_key land in skipped_mask, not in used_mask, and the render is that of the other entries"""
    images, ent = R.pose_map(3)
    e = ent.copy()
    e[1]["valid"] = 0
    out, cover, rec = R.ref_render(rref, images, e, np.eye(3), 320, 224, MEAN)
    assert (rec[0]["used_mask"], rec[0]["skipped_mask"]) == (0b101, 0b010) and rec[0]["n"][1] == 0
    e = ent.copy()
    e[2]["h_origin_key"] = [[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]]
    out2, cover2, rec2 = R.ref_render(rref, images, e, np.eye(3), 320, 224, MEAN)
    assert (rec2[0]["used_mask"], rec2[0]["skipped_mask"]) == (0b011, 0b100) and rec2[0]["n"][2] == 0
    two, cover_two, rec_two = R.ref_render(rref, images[:2], ent[:2], np.eye(3), 320, 224, MEAN)
    assert out2.tobytes() == two.tobytes() and cover2.tobytes() == cover_two.tobytes() and rec2[0]["sse"].tolist() == rec_two[0]["sse"].tolist()
    # no valid entry at all: zeros, and a record that is zero but for the view and skipped_mask
    e = ent.copy()
    e["valid"] = 0
    out, cover, rec = R.ref_render(rref, images, e, R.shift(1.0, 2.0), 50, 37, FEW)
    want = np.zeros(1, R.REC)
    want["h_origin_view"], want["skipped_mask"] = R.shift(1.0, 2.0), 0b111
    assert not out.any() and not cover.any() and rec.tobytes() == want.tobytes()


def test_fit_view(rref):
    images, ent = R.pose_map(8)
    for (w, h, margin) in ((640, 448, 10.0), (200, 300, 0.0), (320, 224, 16.5)):
        v = R.ref_fit_view(rref, ent, w, h, margin)
        assert v is not None and v[0, 0] == v[1, 1] > 0 and v[0, 1] == v[1, 0] == v[2, 0] == v[2, 1] == 0 and v[2, 2] == 1
        pts = []
        for e in ent:
            q = np.concatenate([synth.P4, np.ones((4, 1))], axis=1) @ (v @ np.linalg.inv(e["h_origin_key"])).T
            pts.append(q[:, :2] / q[:, 2:])
        pts = np.concatenate(pts)
        tol = 1e-9 * max(w, h)
        assert pts[:, 0].min() >= margin - tol and pts[:, 0].max() <= w - 1 - margin + tol
        assert pts[:, 1].min() >= margin - tol and pts[:, 1].max() <= h - 1 - margin + tol
        touch_x = abs(pts[:, 0].min() - margin) <= tol and abs(pts[:, 0].max() - (w - 1 - margin)) <= tol
        touch_y = abs(pts[:, 1].min() - margin) <= tol and abs(pts[:, 1].max() - (h - 1 - margin)) <= tol
        assert touch_x or touch_y
        # centred on the other axis
        assert abs((pts[:, 0].min() - margin) - (w - 1 - margin - pts[:, 0].max())) <= tol and abs((pts[:, 1].min() - margin) - (h - 1 - margin - pts[:, 1].max())) <= tol
    # an invalid entry does not count: the view of entry 0 alone is the frame scaled into the view
    e = ent.copy()
    e["valid"][1:] = 0
    v = R.ref_fit_view(rref, e, 320, 224, 0.0)
    assert v is not None and np.abs(v - np.eye(3)).max() <= 1e-12
    e["valid"] = 0
    assert R.ref_fit_view(rref, e, 320, 224, 0.0) is None                                 # an empty map
    assert R.ref_fit_view(rref, ent, 21, 224, 10.0) is None                               # no room between the margins
    assert R.ref_fit_view(rref, ent, 320, 224, np.nan) is None
    behind = R.entries([np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.01, 0.0, 1.0]])])  # its inverse puts corners at z <= 0
    assert R.ref_fit_view(rref, behind, 320, 224, 0.0) is None


def test_texture_map_ranks(rref):
    """three keyframes cut from one texture: with exact matrices every entry's sse / n in MEAN mode lies below its value when entry 1's matrix is
    displaced by 2 px, and the displaced entry then has the largest (the GPU test asserts the same on the device's records)"""
    images, exact, off = R.texture_map()
    _, cover, a = R.ref_render(rref, images, exact, np.eye(3), 320, 224, MEAN)
    _, _, b = R.ref_render(rref, images, off, np.eye(3), 320, 224, MEAN)
    assert (cover == 3).sum() > 20000 and a[0]["n_overlap"] > 50000
    R.check_ranks(a, b)
