"""A keyframe map rendered into a view on the device (include/hnet.h hnet_op_keyframe_render; csrc/kernels_keyframe_render.hip): image, cover
and record byte for byte the host reference's (tests/cpp/keyframe_render_ref.cpp compiles the header the device compiles), three properties that do not
go through the restated rule, the refusals of the operator-level call, and the independence of a sessions render from n, slot and run."""
import ctypes as C

import numpy as np
import pytest

import keyframe_map_util as M
import keyframe_render_util as R
import keyframe_util as K
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

INVALID = 1
FEW, NEW, MEAN = R.MODES


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return R.build_ref(tmp_path_factory.mktemp("keyframe_render_ref_gpu"))


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


@pytest.mark.parametrize("size", R.VIEWS)
@pytest.mark.parametrize("m", (1, 3, 8))
def test_bit_for_bit(eng, rref, m, size):
    """image, cover and record equal the host reference's byte for byte, in the three modes"""
    w, h = size
    images, ent = R.pose_map(m)
    for mode in R.MODES:
        dev = eng.op_keyframe_render(images, ent, R.view(w, h), w, h, mode)
        _same(dev, R.ref_render(rref, images, ent, R.view(w, h), w, h, mode), (m, size, mode))
        if m > 1 and size == (320, 224):
            assert dev[2][0]["n_overlap"] > 10000 and dev[2][0]["used_mask"] == (1 << m) - 1          # the case does overlap


@pytest.mark.parametrize("m", (3, 8))
def test_skipped_entries(eng, rref, m):
    """a map with an invalid entry in the middle and one with a singular h_origin_key: both land in skipped_mask and not in used_mask, and everything
    equals the host reference's"""
    images, ent = R.pose_map(m)
    mid, last, full = m // 2, m - 1, (1 << m) - 1
    e = ent.copy()
    e[mid]["valid"] = 0
    e[last]["h_origin_key"] = [[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]]
    for size in ((320, 224), (50, 37)):
        for mode in R.MODES:
            dev = eng.op_keyframe_render(images, e, R.view(*size), *size, mode)
            _same(dev, R.ref_render(rref, images, e, R.view(*size), *size, mode), (m, size, mode))
            r = dev[2][0]
            assert r["skipped_mask"] == (1 << mid) | (1 << last) and r["used_mask"] == full & ~r["skipped_mask"]
            assert r["n"][mid] == 0 and r["n"][last] == 0
    # no entry takes part: zeros, and a record that is zero but for the view and skipped_mask
    e = ent.copy()
    e["valid"] = 0
    img, cover, rec = eng.op_keyframe_render(images, e, R.view(50, 37), 50, 37, FEW)
    want = np.zeros(1, R.REC)
    want["h_origin_view"], want["skipped_mask"] = R.view(50, 37), full
    assert not img.any() and not cover.any() and rec.tobytes() == want.tobytes()


def test_identity_view_returns_the_image(eng):
    """property 1: an identity view of a one-entry map at 320 x 224 is the stored image, cover all 1, no overlap"""
    images, _ = R.pose_map(3)
    for mode in R.MODES:
        img, cover, rec = eng.op_keyframe_render(images[2:3], R.entries([np.eye(3)]), np.eye(3), 320, 224, mode)
        assert img.tobytes() == images[2].tobytes() and (cover == 1).all()
        r = rec[0]
        assert (r["n_covered"], r["n_overlap"], r["used_mask"], r["skipped_mask"]) == (71680, 0, 1, 0) and not r["n"].any() and not r["sse"].any()


@pytest.mark.parametrize("shift", ((37, -20), (-64, 15), (5, 223), (-319, 0)))
def test_integer_translation(eng, shift):
    """property 2: a view that is an integer translation of the origin returns the shifted image, zeros and cover 0 outside it"""
    dx, dy = shift
    images, _ = R.pose_map(3)
    src = images[1]
    img, cover, rec = eng.op_keyframe_render(src[None], R.entries([np.eye(3)]), R.shift(dx, dy), 320, 224, FEW)
    want, wcover = np.zeros((224, 320), np.uint8), np.zeros((224, 320), np.uint8)
    # view pixel (u, v) shows origin pixel (u - dx, v - dy)
    u0, u1, v0, v1 = max(dx, 0), min(320 + dx, 320), max(dy, 0), min(224 + dy, 224)
    want[v0:v1, u0:u1] = src[v0 - dy:v1 - dy, u0 - dx:u1 - dx]
    wcover[v0:v1, u0:u1] = 1
    assert img.tobytes() == want.tobytes() and cover.tobytes() == wcover.tobytes()
    assert rec[0]["n_covered"] == int(wcover.sum()) > 0 and rec[0]["n_overlap"] == 0


def test_displaced_entry_stands_out(eng, rref):
    """property 3: three keyframes cut from one texture by known homographies.  With exact h_origin_key every entry's sse / n in MEAN mode lies below
    its value when entry 1's matrix is displaced by 2 px, and the displaced entry then has the largest of the three: inequalities and ranks, checked on
    the host reference first (tests/test_keyframe_render_rule.py::test_texture_map_ranks is the same check without a GPU)"""
    images, exact, off = R.texture_map()
    R.check_ranks(R.ref_render(rref, images, exact, np.eye(3), 320, 224, MEAN)[2], R.ref_render(rref, images, off, np.eye(3), 320, 224, MEAN)[2])
    a = eng.op_keyframe_render(images, exact, np.eye(3), 320, 224, MEAN)[2]
    b = eng.op_keyframe_render(images, off, np.eye(3), 320, 224, MEAN)[2]
    R.check_ranks(a, b)


def test_op_refusals(eng):
    """every refusal of the operator-level call returns HNET_ERR_INVALID_ARG and writes nothing"""
    L = _capi.lib()
    images, ent = R.pose_map(8)
    big = np.concatenate([images, images[:1]])
    ent9 = np.concatenate([ent, ent[:1]])
    view = np.eye(3)
    out, cover, rec = np.full(64, 0xA5, np.uint8), np.full(64, 0xA5, np.uint8), np.full(224, 0xA5, np.uint8)

    def call(m=3, img=images, e=ent, v=view, o=(8, 8, 0), outp=out, coverp=cover, recp=rec, ctx=eng.handle):
        oo = None if o is None else _capi.KeyframeRenderOpts(o[0], o[1], o[2], 0)
        p = lambda a: None if a is None else a.ctypes.data                     # noqa: E731
        return L.hnet_op_keyframe_render(ctx, m, p(img), p(e), p(v), C.addressof(oo) if oo is not None else None, p(outp), p(coverp), p(recp))
    assert call(ctx=None) == INVALID
    assert call(m=0) == INVALID and call(m=9, img=big, e=ent9) == INVALID and call(m=-1) == INVALID
    for o in ((0, 8, 0), (8, 0, 0), (-1, 8, 0), (8193, 8, 0), (8, 8193, 0), (8, 8, 3), (8, 8, -1), None):
        assert call(o=o) == INVALID, o
    for k, bad in ((0, np.nan), (4, np.inf), (8, -np.inf)):
        v = np.eye(3)
        v.reshape(9)[k] = bad
        assert call(v=v) == INVALID
    assert call(img=None) == INVALID and call(e=None) == INVALID and call(v=None) == INVALID
    assert call(outp=None) == INVALID and call(coverp=None) == INVALID and call(recp=None) == INVALID
    assert (out == 0xA5).all() and (cover == 0xA5).all() and (rec == 0xA5).all()
    assert call() == 0 and not (rec == 0xA5).all()                              # and the call they were variations of is good


def test_independence(eng):
    """the record, image and cover of a session do not depend on n, slot or run: session 2 rendered alone, as slot 0 of 3 and as slot 2 of 3, twice each,
    gives equal bytes; and the operator-level call twice"""
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
        views = {c: R.shift(3.0 + c, -2.0) @ np.diag([0.9, 0.9, 1.0]) for c in cams}
        got = []
        for ids in ([2], [2, 0, 1], [1, 0, 2], [2], [2, 1, 0], [0, 1, 2]):
            img, cover, rec = s.keyframe_render(ids, 200, 150, np.stack([views[c] for c in ids]), MEAN)
            k = ids.index(2)
            got.append((img[k].tobytes(), cover[k].tobytes(), rec[k].tobytes()))
            assert rec[k]["n_overlap"] > 1000 and bin(rec[k]["used_mask"]).count("1") >= 3
        assert all(g == got[0] for g in got[1:])
    finally:
        s.close()
    images, ent = R.pose_map(8)
    a, b = eng.op_keyframe_render(images, ent, R.view(320, 224), 320, 224, MEAN), eng.op_keyframe_render(images, ent, R.view(320, 224), 320, 224, MEAN)
    _same(a, b, "twice")
