"""The keyframe render on the device at hostile views and far from the origin (include/hnet.h hnet_op_keyframe_render, hnet_sessions_keyframe_render;
csrc/kernels_keyframe_render.hip): the cases of tests/keyframe_render_hostile.py.  Every case is first shown to be what its name says on the
host reference (tests/cpp/keyframe_render_ref.cpp), then the device's image, cover and record are asserted equal to that reference byte for byte; the
one-entry renders are also held against the plain numpy reference and the m-entry renders against the restated composite, neither of which reads the
header; the counters beyond 2^32 against their closed forms."""
import ctypes as C
import functools

import numpy as np
import pytest

import keyframe_map_util as M
import keyframe_render_hostile as H
import keyframe_render_util as R
import keyframe_util as K
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

FEW, NEW, MEAN = R.MODES


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return R.build_ref(tmp_path_factory.mktemp("keyframe_render_hostile_ref_gpu"))


@pytest.fixture(scope="module")
def render(rref):
    return functools.partial(R.ref_render, rref)


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=8)
    yield e
    e.close()


def _same(dev, ref, what):
    (img, cover, rec), (rimg, rcover, rrec) = dev, ref
    assert rec.tobytes() == rrec.tobytes(), (what, rec, rrec)
    assert cover.tobytes() == rcover.tobytes(), (what, int((cover != rcover).sum()))
    assert img.tobytes() == rimg.tobytes(), (what, int((img != rimg).sum()))


# ---- A. references that do not read the header

@pytest.mark.parametrize("name", list(H.PLAIN_VIEWS))
def test_plain_reference(eng, name):
    """cover equality and the byte tolerance of the device's one-entry renders under the three comparison views"""
    view, w, h, which = H.PLAIN_VIEWS[name]
    images, ent = R.pose_map(3)
    for j in which:
        img, cover, rec = eng.op_keyframe_render(images[j:j + 1], ent[j:j + 1], view, w, h, FEW)
        share, worst = H.check_plain(img, cover, images[j], ent[j]["h_origin_key"], view, w, h)
        print(f"device, {name} entry {j}: excluded share {share:.2e}, largest |byte - plain| {worst:.5f}, covered {int(cover.sum())}")
        assert rec[0]["n_covered"] == cover.sum() > 0


@pytest.mark.parametrize("which", ("m3", "m8", "tie"))
def test_composite(eng, render, which):
    """the m-entry render equals the integer composite of the device's own one-entry renders in the three modes, and the host reference"""
    images, ent = H.tie_map() if which == "tie" else R.pose_map(int(which[1:]))
    H.check_composite(eng.op_keyframe_render, images, ent, R.view(320, 224), 320, 224)
    for mode in R.MODES:
        _same(eng.op_keyframe_render(images, ent, R.view(320, 224), 320, 224, mode), render(images, ent, R.view(320, 224), 320, 224, mode), (which, mode))


# ---- B 1. the counters

@pytest.mark.parametrize("name", list(H.COUNTER_CASES))
def test_counter_width(eng, render, name):
    """sums beyond 2^32 and the largest sum of one workgroup: the closed forms, and the host reference"""
    m, view, w, h, mode, n_cov, n_ov, n, sse = H.COUNTER_CASES[name]
    images, ent = H.flat_map(m)
    dev = eng.op_keyframe_render(images, ent, view, w, h, mode)
    r = dev[2][0]
    assert (r["n_covered"], r["n_overlap"], r["used_mask"], r["skipped_mask"]) == (n_cov, n_ov, (1 << m) - 1, 0) and (dev[1] == m).all()
    assert r["n"].tolist() == n and r["sse"].tolist() == sse, (r["n"], r["sse"])
    _same(dev, render(images, ent, view, w, h, mode), name)


# ---- B 2. the tile edges

@pytest.mark.parametrize("size", H.TILE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_edges(eng, render, size):
    w, h = size
    images, ent = R.pose_map(3)
    ref = render(images, ent, H.tile_view(w, h), w, h, MEAN)
    assert ref[2][0]["used_mask"] == 7 and ref[2][0]["n_covered"] > 0.5 * w * h
    _same(eng.op_keyframe_render(images, ent, H.tile_view(w, h), w, h, MEAN), ref, size)


@pytest.mark.parametrize("size", H.GUARD_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nothing_past_the_output(eng, render, size):
    """hnet_op_keyframe_render through raw ctypes into buffers 256 bytes longer than the view: the guard bytes are untouched, the view is the reference's"""
    w, h = size
    L = _capi.lib()
    images, ent = R.pose_map(3)
    view = np.ascontiguousarray(H.tile_view(w, h))
    o = _capi.KeyframeRenderOpts(w, h, MEAN, 0)
    out, cover = np.full(w * h + H.GUARD_BYTES, H.GUARD_FILL, np.uint8), np.full(w * h + H.GUARD_BYTES, H.GUARD_FILL, np.uint8)
    rec = np.full(R.REC.itemsize + H.GUARD_BYTES, H.GUARD_FILL, np.uint8)
    assert L.hnet_op_keyframe_render(eng.handle, 3, images.ctypes.data, ent.ctypes.data, view.ctypes.data, C.addressof(o), out.ctypes.data, cover.ctypes.data,
                                     rec.ctypes.data) == 0
    assert (out[w * h:] == H.GUARD_FILL).all() and (cover[w * h:] == H.GUARD_FILL).all() and (rec[R.REC.itemsize:] == H.GUARD_FILL).all()
    rimg, rcover, rrec = render(images, ent, view, w, h, MEAN)
    assert out[:w * h].tobytes() == rimg.tobytes() and cover[:w * h].tobytes() == rcover.tobytes() and rec[:R.REC.itemsize].tobytes() == rrec.tobytes()


# ---- B 3. hostile views and entries

@pytest.mark.parametrize("name", list(H.VIEWS))
def test_hostile_views(eng, render, name):
    view, w, h = H.VIEWS[name]
    images, ent = H.identity_first()
    ref = H.check_view(name, render)
    for mode in R.MODES:
        _same(eng.op_keyframe_render(images, ent, view, w, h, mode), ref[mode], (name, mode))
    if name in H.EXACT_IMAGES:                                              # the one-entry identity map, on the device itself
        img, cover, _ = eng.op_keyframe_render(images[2:3], R.entries([np.eye(3)]), view, w, h, FEW)
        assert img.tobytes() == np.ascontiguousarray(H.EXACT_IMAGES[name](images[2])).tobytes() and (cover == 1).all()


@pytest.mark.parametrize("name", list(H.VIEWS))
def test_hostile_entries(eng, render, name):
    images, e = H.hostile_entries(name)
    view, w, h, _ = H.PLAIN_VIEWS["turned"]
    ref = H.check_entry(name, render)
    for mode in R.MODES:
        _same(eng.op_keyframe_render(images, e, view, w, h, mode), ref[mode], (name, mode))


def test_sessions_refused_slot_beside_good_ones(eng):
    """3 cameras tracked over 5 frames; one call renders a good view, a refused view and the horizon view: every slot equals the operator on that session's
    map read back, and the good slot's bytes are those of a call in which all three views are good"""
    from cuahn_vio_amd.homography_net import HnetSessions
    s = HnetSessions(eng, 4)
    try:
        s.enable_keyframes()
        s.enable_keyframe_map(4)
        s.enable_keyframe_render(320, 224)
        kw = K.opts_kw(K.opts(**M.TRACK_OPTS))
        seqs = [K.sequence("out-and-back", seed) for seed in (1, 2, 5)]
        cams = [0, 1, 2]
        for i in range(5):
            s.push(cams, np.stack([q[0][i] for q in seqs]))
            s.keyframe_track(cams, np.stack([q[2][i] for q in seqs]), **kw)
        maps = {c: (np.stack([s.map_keyframe(c, j) for j in range(4)]), s.keyframe_map_info(c)[0]) for c in cams}
        good = R.shift(3.0, -2.0) @ np.diag([0.9, 0.9, 1.0])
        hostile = np.stack([good, H.VIEWS["near-singular-refused"][0], H.VIEWS["horizon"][0]])
        for mode in R.MODES:
            img, cover, rec = s.keyframe_render(cams, 320, 224, hostile, mode)
            for k, c in enumerate(cams):
                oi, oc, orec = eng.op_keyframe_render(maps[c][0], maps[c][1], hostile[k], 320, 224, mode)
                assert rec[k].tobytes() == orec[0].tobytes(), (mode, c, rec[k], orec[0])
                assert img[k].tobytes() == oi.tobytes() and cover[k].tobytes() == oc.tobytes(), (mode, c)
            assert rec[0]["used_mask"] == 15 and rec[0]["n_overlap"] > 1000
            assert (rec[1]["used_mask"], rec[1]["skipped_mask"]) == (0, 15) and not img[1].any() and not cover[1].any()
            assert rec[1].tobytes() == H.zero_record(hostile[1], 15)[0].tobytes()
            assert rec[2]["used_mask"] == 15 and 0 < rec[2]["n_covered"] < 320 * 224
            img2, cover2, rec2 = s.keyframe_render(cams, 320, 224, np.stack([good] * 3), mode)
            assert img2[0].tobytes() == img[0].tobytes() and cover2[0].tobytes() == cover[0].tobytes() and rec2[0].tobytes() == rec[0].tobytes()
            assert rec2[1]["used_mask"] == 15 and rec2[1]["n_covered"] > 0
    finally:
        s.close()


# ---- B 5. far from the origin

def test_far_map_renders_as_at_the_origin(eng, render):
    """pose_map(3) with every h_origin_key moved 100 000 px from the origin under a view moved the same way: on the reference the unmoved render byte for
    byte, on the device the reference, used_mask 7"""
    images, e, view = H.far_map()
    ref = H.check_far(render)
    for mode in R.MODES:
        dev = eng.op_keyframe_render(images, e, view, 320, 224, mode)
        assert dev[2][0]["used_mask"] == 7
        _same(dev, ref[mode], mode)
