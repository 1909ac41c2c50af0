"""The three layers on a keyframe map - render, adjust, localise (include/hnet.h; csrc/capi_keyframe_render.hip, capi_keyframe_adjust.hip,
capi_keyframe_localise.hip) - enabled TOGETHER on one store (csrc/keyframes_internal.h): they share the store's event pair, its alignment scratch, the
frame of a call and the owner of their buffers.  Sessions objects of 2 cameras with maps of capacity 2 and two stored keyframes each (the first two
frames of keyframe_adjust_util.path_frames, every frame a keyframe) on a context of max_batch 8.  Three reference objects enable one layer each; one
object enables all three in the order render, adjust, localise and one in the reverse order; on each of those a render, an adjustment without apply and a
localise without apply return the bytes of the reference objects, every call leaves a device time and no hnet_timing; then both are destroyed, made again
in the same process with everything enabled, and render the same bytes once more."""
import numpy as np
import pytest

import keyframe_adjust_util as A
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

N_CAM, CAP, SEEDS = 2, 2, (2, 4)
W, H = 96, 64
LAYERS = ("render", "adjust", "localise")
IDS = [1, 0]
KW = dict(A.TEXTURE_OPTS)


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=8)
    yield e
    e.close()


def _fleet(eng, layers):
    """a sessions object with `layers` enabled in that order, both cameras tracked over two frames"""
    from cuahn_vio_amd.homography_net import HnetSessions
    s = HnetSessions(eng, N_CAM)
    try:
        s.enable_keyframes()
        s.enable_keyframe_map(CAP)
        for name in layers:
            if name == "render":
                s.enable_keyframe_render(W, H)
            else:
                getattr(s, "enable_keyframe_" + name)()
        seqs = [A.path_frames(seed) for seed in SEEDS]
        cams = list(range(N_CAM))
        for i in range(CAP):
            s.push(cams, np.stack([q[0][i] for q in seqs]))
            s.keyframe_track(cams, np.stack([q[2][i] for q in seqs]), **A.TRACK_KW)
    except BaseException:
        s.close()
        raise
    return s


def _timed(s, call):
    """call() on s -> the bytes of everything it returned; it leaves a device time of its own and every hnet_timing as it was"""
    before = s.last_timing()
    out = call()
    assert s.last_keyframe_device_ms() > 0.0
    assert s.last_timing() == before
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (out if isinstance(out, tuple) else (out,)))


def _calls(s, views):
    return {"render": lambda: s.keyframe_render(IDS, W, H, views, _capi.RENDER_MEAN),
            "adjust": lambda: s.keyframe_adjust(IDS, want_edge_records=True, apply=0, **KW),
            "localise": lambda: s.keyframe_localise(IDS, apply=0, max_iterations=6)}


@pytest.fixture(scope="module")
def reference(eng):
    """the views of the render, and per layer the bytes a sessions object with only that layer returns: computed once, read by every test"""
    want, views = {}, None
    for name in LAYERS:
        s = _fleet(eng, (name,))
        try:
            if views is None:
                ent = [s.keyframe_map_info(c)[0] for c in IDS]
                assert all(int(e["valid"].sum()) == CAP for e in ent), "two stored keyframes each"
                views = np.stack([_capi.keyframe_render_fit_view(e, W, H, 2.0) for e in ent])
                views.setflags(write=False)
            out = _calls(s, views)[name]()
            if name == "render":
                assert (out[2]["used_mask"] == 3).all() and out[1].any()
            elif name == "adjust":
                assert (out[0]["n_jobs"] == 1).all()
            else:
                print("localise flags", out["flags"], "used", out["used_mask"], "cover", out["cover"])
            want[name] = _timed(s, _calls(s, views)[name])
            assert want[name] == b"".join(np.ascontiguousarray(a).tobytes() for a in (out if isinstance(out, tuple) else (out,))), "a repeated call"
        finally:
            s.close()
    return views, want


def test_layers_together_in_both_orders_and_again(eng, reference):
    """render, adjust (apply = 0), localise (apply = 0) on an object with the three layers enabled in that order and on one with the reverse order: the
    bytes of the objects with one layer each; after both are destroyed and made again with everything enabled, the render's bytes once more"""
    views, want = reference
    fleets = []
    try:
        for order in (LAYERS, LAYERS[::-1]):
            fleets.append(_fleet(eng, order))
        for s, order in zip(fleets, (LAYERS, LAYERS[::-1])):
            calls = _calls(s, views)
            for name in LAYERS:
                assert _timed(s, calls[name]) == want[name], (order, name)
        while fleets:
            fleets.pop().close()
        for order in (LAYERS, LAYERS[::-1]):
            fleets.append(_fleet(eng, order))
        for s, order in zip(fleets, (LAYERS, LAYERS[::-1])):
            assert _timed(s, _calls(s, views)["render"]) == want["render"], (order, "again")
    finally:
        for s in fleets:
            s.close()
