"""hnet_sessions_keyframe_render on the device (include/hnet.h; csrc/capi_keyframe_render.hip): a map built by tracking a short synthetic
sequence renders like hnet_op_keyframe_render on the images and entries read back from the session, a NULL view is the current frame's, every refusal
returns its code and changes nothing, and a sessions object that enabled the render but never called it tracks and revisits as one without it.
Sessions objects of 4 cameras on a context of max_batch 8; the tracks re-key at every frame (keyframe_map_util.TRACK_OPTS)."""
import ctypes as C

import numpy as np
import pytest

import keyframe_map_util as M
import keyframe_render_util as R
import keyframe_util as K
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, CAPACITY = 1, 4, 5
N_CAM, CAP = 4, 4
TRACK_KW = K.opts_kw(K.opts(**M.TRACK_OPTS))
FEW, NEW, MEAN = R.MODES


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

    def make(render=(320, 224), keymap=True):
        s = HnetSessions(eng, N_CAM)
        s.enable_keyframes()
        if keymap:
            s.enable_keyframe_map(CAP)
        if render:
            s.enable_keyframe_render(*render)
        made.append(s)
        return s
    yield make
    for s in made:
        s.close()


def _track(s, cams, seeds, upto):
    """frames 0 .. upto - 1 of out-and-back(seed) on each camera -> the last call's records"""
    seqs = [K.sequence("out-and-back", seed) for seed in seeds]
    out = None
    for i in range(upto):
        s.push(cams, np.stack([q[0][i] for q in seqs]))
        out = s.keyframe_track(cams, np.stack([q[2][i] for q in seqs]), **TRACK_KW)
    return out


def _map(s, cam):
    entries, _ = s.keyframe_map_info(cam)
    return np.stack([s.map_keyframe(cam, j) for j in range(CAP)]), entries


def _keyframe(s, cam):
    try:
        return s.keyframe(cam).tobytes()
    except _capi.HnetError as e:                                               # (a session without a keyframe)
        assert e.status == NOT_READY
        return None


def _snapshot(s, cam):
    """everything the sessions and the keyframe layers hold of a session"""
    images, entries = _map(s, cam)
    frame = s.frame(cam, 1).tobytes() if s.image_count(cam) else None
    return images.tobytes(), entries.tobytes(), s.keyframe_map_info(cam)[1].tobytes(), _keyframe(s, cam), frame, s.image_count(cam)


def test_equals_the_operator(eng, fleet):
    """two cameras tracked over 6 and one over 2 frames; each session's render equals hnet_op_keyframe_render on its images and entries read back, byte
    for byte, for a view of its own per session, two sizes and the three modes; a session without a keyframe renders zeros"""
    s = fleet()
    _track(s, [0, 2], (1, 2), 6)
    _track(s, [3], (5,), 2)
    s.push([1], K.sequence("out-and-back", 11)[0][:1])                      # camera 1: an image, no keyframe, an empty map
    maps = {c: _map(s, c) for c in range(N_CAM)}
    assert [int(maps[c][1]["valid"].sum()) for c in range(N_CAM)] == [4, 0, 4, 2]
    ids = [2, 1, 3, 0]
    for (w, h) in ((320, 224), (50, 37)):
        views = np.stack([_capi.keyframe_render_fit_view(maps[c][1], w, h, 2.0) if c != 1 else R.shift(c, 1.0) for c in ids])
        for mode in R.MODES:
            img, cover, rec = s.keyframe_render(ids, w, h, views, mode)
            for k, c in enumerate(ids):
                oi, oc, orec = eng.op_keyframe_render(maps[c][0], maps[c][1], views[k], w, h, mode)
                assert rec[k].tobytes() == orec[0].tobytes(), (w, h, mode, c)
                assert img[k].tobytes() == oi.tobytes() and cover[k].tobytes() == oc.tobytes(), (w, h, mode, c)
            k = ids.index(1)
            want = np.zeros(1, R.REC)
            want["h_origin_view"], want["skipped_mask"] = views[k], (1 << CAP) - 1
            assert not img[k].any() and not cover[k].any() and rec[k].tobytes() == want[0].tobytes()
            assert rec[ids.index(0)]["n_overlap"] > 0 and rec[ids.index(0)]["used_mask"] == 15 and rec[ids.index(3)]["used_mask"] == 3
    assert s.last_keyframe_device_ms() > 0.0


def test_null_view_is_the_current_frame(fleet):
    """with a NULL view the record's view is the h_origin_curr of the last track's record, and the render lies closer (mean squared difference over the
    covered pixels) to the current frame than to that frame shifted by 8 px"""
    s = fleet()
    last = _track(s, [1, 3], (2, 5), 6)
    img, cover, rec = s.keyframe_render([3, 1], 320, 224, None, FEW)
    for k, (c, t) in enumerate(((3, last[1]), (1, last[0]))):
        assert rec[k]["h_origin_view"].tobytes() == t["h_origin_curr"].tobytes()
        frame = s.frame(c, 1).astype(np.float64)
        shifted = np.roll(frame, 8, axis=1)
        on = cover[k] >= 1
        on[:, :8] = False                                                       # (the columns the roll wrapped)
        assert on.sum() > 50000
        near, far = ((img[k][on] - frame[on]) ** 2).mean(), ((img[k][on] - shifted[on]) ** 2).mean()
        print("camera", c, "mse to the current frame", near, "to the frame shifted by 8 px", far)
        assert near < far
    # the same through an explicit view
    img2, cover2, rec2 = s.keyframe_render([3, 1], 320, 224, rec["h_origin_view"], FEW)
    assert img2.tobytes() == img.tobytes() and cover2.tobytes() == cover.tobytes() and rec2.tobytes() == rec.tobytes()


def test_refusals_change_nothing(eng, fleet):
    """every refusal returns its code, writes nothing into the output buffers and leaves states, entries and images as they were"""
    L = _capi.lib()
    frames = K.sequence("out-and-back", 11)[0]
    never, nomap, a = fleet(render=None), fleet(render=None, keymap=False), fleet(render=(100, 80))
    out, cover, rec = np.full(9 * 100 * 80, 0xA5, np.uint8), np.full(9 * 100 * 80, 0xA5, np.uint8), np.full(9 * 224, 0xA5, np.uint8)
    eye9 = np.tile(np.eye(3).reshape(9), (9, 1))

    def call(s, ids, v=eye9, o=(100, 80, 0), outp=out, coverp=cover, recp=rec):
        ids = np.asarray(ids, np.int32)
        oo = None if o is None else _capi.KeyframeRenderOpts(o[0], o[1], o[2], 0)
        p = lambda x: None if x is None else x.ctypes.data                     # noqa: E731
        return L.hnet_sessions_keyframe_render(s._s if s is not None else None, len(ids), ids.ctypes.data, p(v), C.addressof(oo) if oo is not None else None,
                                               p(outp), p(coverp), p(recp))
    # the enable: before the map, twice, a maximum out of range
    assert L.hnet_sessions_enable_keyframe_render(None, 10, 10) == INVALID and L.hnet_sessions_enable_keyframe_render(nomap._s, 10, 10) == INVALID
    assert L.hnet_sessions_enable_keyframe_render(a._s, 10, 10) == INVALID
    for bad in ((0, 10), (10, 0), (8193, 10), (10, 8193), (-5, 10)):
        assert L.hnet_sessions_enable_keyframe_render(never._s, *bad) == INVALID, bad
    _track(a, [0, 1], (1, 2), 3)
    a.push([2], frames[:1])                                                    # an image, no keyframe
    a.push([1], frames[4:5])                                                   # an image its last track did not see
    snap = {c: _snapshot(a, c) for c in range(N_CAM)}
    assert call(never, [0]) == INVALID and call(nomap, [0]) == INVALID and call(None, [0]) == INVALID        # before the enable
    assert call(a, [0, 0]) == INVALID and call(a, [4]) == INVALID and call(a, [-1]) == INVALID and call(a, []) == INVALID
    assert call(a, [0, 1, 2, 3, 0, 1, 2, 3, 0]) == CAPACITY
    for o in ((0, 80, 0), (100, 0, 0), (101, 80, 0), (100, 81, 0), (100, 80, 3), (100, 80, -1), None):
        assert call(a, [0], o=o) == INVALID, o
    for k, bad in ((0, np.nan), (13, np.inf)):
        v = eye9.copy()
        v.reshape(-1)[k] = bad
        assert call(a, [0, 3], v=v) == INVALID
    assert call(a, [0], outp=None) == INVALID and call(a, [0], coverp=None) == INVALID and call(a, [0], recp=None) == INVALID
    # a NULL view: a session without a keyframe (2, and 3 without an image), and one whose latest image no track saw (1)
    assert call(a, [0, 2], v=None) == NOT_READY and call(a, [0, 3], v=None) == NOT_READY and call(a, [0, 1], v=None) == NOT_READY
    assert (out == 0xA5).all() and (cover == 0xA5).all() and (rec == 0xA5).all()
    for c in range(N_CAM):
        assert _snapshot(a, c) == snap[c], c
    # and what they were variations of is good: with views every session renders (those without a keyframe as zeros), with NULL the tracked one
    assert call(a, [0, 1, 2, 3]) == 0 and call(a, [0], v=None) == 0
    for c in range(N_CAM):
        assert _snapshot(a, c) == snap[c], c


def test_enabled_but_never_called_changes_nothing(fleet):
    """a sessions object with the render enabled and never called, and one that renders between the calls, return track and revisit records byte for
    byte equal to one without the render; the render leaves everything the sessions hold as it was"""
    plain, enabled, used = fleet(render=None), fleet(), fleet()
    frames, _, steps = K.sequence("out-and-back", 5)
    ids = [1, 3]
    attached = 0
    for i in range(7):
        recs = []
        for s in (plain, enabled, used):
            s.push(ids, np.stack([frames[i], frames[i + 1]]))
            recs.append(s.keyframe_track(ids, np.stack([steps[i], steps[i + 1]]), **TRACK_KW))
        assert recs[0].tobytes() == recs[1].tobytes() == recs[2].tobytes(), i
        snap = {c: _snapshot(used, c) for c in ids}
        used.keyframe_render(ids, 320, 224, None, MEAN)
        used.keyframe_render(ids[::-1], 64, 48, np.stack([np.eye(3), R.shift(5.0, 5.0)]), NEW)
        for c in ids:
            assert _snapshot(used, c) == snap[c], (i, c)
        if i >= 4:
            rv = [s.keyframe_revisit(ids, **M.opts_kw(M.opts())) for s in (plain, enabled, used)]
            assert rv[0].tobytes() == rv[1].tobytes() == rv[2].tobytes(), i
            attached += int((rv[0]["flags"] == _capi.RV_ATTACHED).sum())
    assert attached >= 1
    for c in ids:
        assert _snapshot(plain, c) == _snapshot(enabled, c) == _snapshot(used, c)
