"""The cases of tests/keyframe_render_hostile.py on the host reference, no GPU (tests/cpp/keyframe_render_ref.cpp, keyframe_map_ref.cpp): the
header against the plain numpy reference and the restated composite, the closed forms of the counters beyond 2^32, the tile-edge sizes, every hostile
view and entry with the condition that shows it is what its name says, the refusals of render_fit_view and of its C entry, and the domain of the one
inverse far from the origin."""
import ctypes as C
import functools

import numpy as np
import pytest

import keyframe_map_util as M
import keyframe_render_hostile as H
import keyframe_render_util as R
from cuahn_vio_amd import _capi

FEW, NEW, MEAN = R.MODES


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return R.build_ref(tmp_path_factory.mktemp("keyframe_render_hostile_ref"))


@pytest.fixture(scope="module")
def mref(tmp_path_factory):
    return M.build_ref(tmp_path_factory.mktemp("keyframe_map_far_ref"))


@pytest.fixture(scope="module")
def render(rref):
    return functools.partial(R.ref_render, rref)


# ---- A. the header against references that do not read it

@pytest.mark.parametrize("name", list(H.PLAIN_VIEWS))
def test_plain_reference(render, name):
    """cover equality and the byte tolerance of every one-entry render of pose_map(3) under the three comparison views"""
    view, w, h, which = H.PLAIN_VIEWS[name]
    images, ent = R.pose_map(3)
    covered = 0
    for j in which:
        img, cover, rec = render(images[j:j + 1], ent[j:j + 1], view, w, h, FEW)
        share, worst = H.check_plain(img, cover, images[j], ent[j]["h_origin_key"], view, w, h)
        print(f"{name} entry {j}: excluded share {share:.2e}, largest |byte - plain| {worst:.5f}, covered {int(cover.sum())}")
        covered += int(cover.sum())
    assert covered > 0


@pytest.mark.parametrize("which", ("m3", "m8", "tie"))
def test_composite(render, which):
    images, ent = H.tie_map() if which == "tie" else R.pose_map(int(which[1:]))
    H.check_composite(render, images, ent, R.view(320, 224), 320, 224)
    if which == "tie":                                                   # the tie rule decides: the lower slot, in both modes, wherever it covers
        one = render(images[:1], ent[:1], R.view(320, 224), 320, 224, FEW)
        for mode in (FEW, NEW):
            img = render(images, ent, R.view(320, 224), 320, 224, mode)[0]
            assert (img[one[1] == 1] == one[0][one[1] == 1]).all()


def test_composite_restates_the_pixel_rule(rref):
    """the numpy composite against the header's render_pixel and seam_add on random pixels, ties included"""
    rng = np.random.default_rng(11)
    for mode in R.MODES:
        for _ in range(200):
            m = int(rng.integers(1, 9))
            vals, mask = rng.integers(0, 256, m), int(rng.integers(0, 1 << m))
            links, serials = rng.integers(0, 3, m), rng.integers(1, 4, m)
            out, cover, n, sse = R.ref_pixel(rref, vals, mask, links, serials, mode)
            c = np.array([(mask >> j) & 1 for j in range(m)]).reshape(m, 1, 1)
            img, cov, n_cov, n_ov, n2, sse2 = H.composite(vals.reshape(m, 1, 1), c, links, serials, mode)
            assert (int(img[0, 0]), int(cov[0, 0])) == (out, cover) and n2.tolist() == n.tolist() and sse2.tolist() == sse.tolist()


# ---- B 1. the counters

@pytest.mark.parametrize("name", list(H.COUNTER_CASES))
def test_counter_width(render, name):
    m, view, w, h, mode, n_cov, n_ov, n, sse = H.COUNTER_CASES[name]
    images, ent = H.flat_map(m)
    img, cover, rec = render(images, ent, view, w, h, mode)
    r = rec[0]
    assert (r["n_covered"], r["n_overlap"], r["used_mask"]) == (n_cov, n_ov, (1 << m) - 1) and (cover == m).all()
    assert r["n"].tolist() == n and r["sse"].tolist() == sse


# ---- B 2. the tile edges

@pytest.mark.parametrize("size", H.TILE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_sizes_cover_something(render, size):
    """every size renders on the reference with all entries used and most of the view covered"""
    w, h = size
    images, ent = R.pose_map(3)
    img, cover, rec = render(images, ent, H.tile_view(w, h), w, h, MEAN)
    assert rec[0]["used_mask"] == 7 and rec[0]["n_covered"] == (cover >= 1).sum() > 0.5 * w * h and cover[0, 0] >= 1


# ---- B 3. hostile views and entries

@pytest.mark.parametrize("name", list(H.VIEWS))
def test_hostile_views(render, name):
    H.check_view(name, render)


@pytest.mark.parametrize("name", list(H.VIEWS))
def test_hostile_entries(render, name):
    H.check_entry(name, render)


def test_half_turn_unshifted_composes_as_documented(rref):
    """diag(-1, -1, 1) has a positive determinant and inverse[8] = 1: S keeps Z = 1 and the view shows the origin's (-u, -v)"""
    s = R.ref_setup(rref, H.VIEWS["half-turn-unshifted"][0], R.entries([np.eye(3)]))
    assert s is not None and s.tobytes() == H.diag(-1, -1).tobytes()


# ---- B 4. render_fit_view and its C entry

# One entry scaled to a point: h_origin_key = diag(s, s, 1) takes the origin's 320 x 224 frame to 1 / s of it.  The inverse refuses s > 1e12 (det = s^2
# against 1e-12 s^3), so the map has no usable entry and there is no box.  At s = 1e11 the box is 3e-9 px wide, still wider than 0 in double: it fits,
# under a scale of 1e11.  A box of exactly no extent cannot come out of an entry the inverse accepts: that needs 2^-53, the rule stops at 1e-12.
POINT, ALMOST_POINT = np.diag([1e13, 1e13, 1.0]), np.diag([1e11, 1e11, 1.0])


def test_fit_view_refusals(rref):
    _, ent = R.pose_map(3)
    assert R.ref_fit_view(rref, ent, 320, 224, 4.0) is not None                            # what the refusals are variations of
    assert not M.np_invertible(POINT) and R.ref_fit_view(rref, R.entries([POINT]), 320, 224, 0.0) is None
    v = R.ref_fit_view(rref, R.entries([ALMOST_POINT]), 320, 224, 0.0)
    assert M.np_invertible(ALMOST_POINT) and v is not None and abs(v[0, 0] / 1e11 - 1.0) <= 1e-9 and np.isfinite(v).all()
    v = R.ref_fit_view(rref, np.concatenate([ent, R.entries([POINT])]), 320, 224, 4.0)      # among good entries the point is left out
    assert v is not None and v.tobytes() == R.ref_fit_view(rref, ent, 320, 224, 4.0).tobytes()
    behind = R.entries([H.persp(0.01, 0.0)])
    assert M.np_invertible(H.persp(0.01, 0.0)) and R.ref_fit_view(rref, behind, 320, 224, 0.0) is None
    assert R.ref_fit_view(rref, np.concatenate([ent, behind]), 320, 224, 0.0) is None       # one corner behind refuses the whole map
    for w, h, margin in ((320, 224, 111.5), (320, 224, 112.0), (320, 224, 1e9), (21, 224, 10.0), (1, 224, 0.0), (320, 1, 0.0), (1, 1, 0.0)):
        assert R.ref_fit_view(rref, ent, w, h, margin) is None, (w, h, margin)
    assert R.ref_fit_view(rref, ent, 320, 224, 111.0) is not None                           # just below half the height
    for margin in (np.nan, np.inf, -np.inf, -1.0):
        assert R.ref_fit_view(rref, ent, 320, 224, margin) is None, margin


def test_fit_view_c_entry_refusals():
    """hnet_keyframe_render_fit_view returns 0 and leaves h_origin_view untouched"""
    L = _capi.lib()
    _, ent = R.pose_map(8)
    ent9 = np.concatenate([ent, ent[:1]])
    h = np.full(9, -7.0)

    def call(e=ent, cap=8, w=320, hh=224, margin=4.0, out=h):
        return L.hnet_keyframe_render_fit_view(None if e is None else e.ctypes.data, cap, w, hh, C.c_double(margin), None if out is None else out.ctypes.data)
    assert call(cap=0) == 0 and call(cap=-1) == 0 and call(e=ent9, cap=9) == 0
    assert call(e=None) == 0 and call(out=None) == 0
    assert call(w=1) == 0 and call(hh=1) == 0 and call(w=0) == 0 and call(hh=-3) == 0
    assert call(margin=112.0) == 0 and call(margin=np.nan) == 0 and call(margin=np.inf) == 0
    assert call(e=R.entries([POINT]), cap=1) == 0 and call(e=R.entries([H.persp(0.01, 0.0)]), cap=1) == 0
    assert (h == -7.0).all()
    assert call() == 1 and h[8] == 1.0 and h[0] == h[4] > 0                                 # and the call they were variations of is good


def _corners_in_view(ent, v):
    pts = []
    for e in ent:
        q = np.concatenate([np.array([[0.0, 0.0], [319.0, 0.0], [319.0, 223.0], [0.0, 223.0]]), np.ones((4, 1))], axis=1) @ (v @ np.linalg.inv(e["h_origin_key"])).T
        pts.append(q[:, :2] / q[:, 2:])
    return np.concatenate(pts)


def test_fit_view_of_a_far_map(rref):
    """the map 100 000 px from its origin fits, and its corners land inside the margins to 1e-9 max(w, h)"""
    _, e, _ = H.far_map()
    for w, h, margin in ((640, 448, 10.0), (200, 300, 0.0)):
        v = R.ref_fit_view(rref, e, w, h, margin)
        assert v is not None
        pts, tol = _corners_in_view(e, v), 1e-9 * max(w, h)
        assert pts[:, 0].min() >= margin - tol and pts[:, 0].max() <= w - 1 - margin + tol
        assert pts[:, 1].min() >= margin - tol and pts[:, 1].max() <= h - 1 - margin + tol
        assert abs(pts[:, 0].min() - margin) <= tol or abs(pts[:, 1].min() - margin) <= tol       # and touches them on one axis


# ---- B 5 / C. far from the origin

def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("t", H.FAR_T)
def test_far_translations_are_accepted(rref, mref, t):
    """a translation of t px as the entry, as the view and as both 5 px apart: render_setup and relative accept it and S and G agree with numpy float64
    to 1e-9 relative"""
    far, near = R.shift(-t, 0.25 * t), R.shift(-t + 5.0, 0.25 * t - 3.0)
    for key, view in ((far, np.eye(3)), (np.eye(3), far), (far, near), (near, far)):
        s = R.ref_setup(rref, view, R.entries([key]))
        want = key @ np.linalg.inv(view)
        assert s is not None and _rel(s, want / want[2, 2]) <= 1e-9, (t, s, want)
        # relative: the current frame at `view`, the stored keyframe at `key`
        g = M.ref_relative(mref, view, R.entries([key])[0])
        want = view @ np.linalg.inv(key)
        assert g is not None and _rel(g[0], want / want[2, 2]) <= 1e-9, (t, g, want)
        assert M.np_relative(view, key) is not None
        assert R.ref_fit_view(rref, R.entries([key]), 320, 224, 2.0) is not None


def test_far_select_counts_the_same_grid(mref):
    """select among entries 100 000 px from the origin finds the candidate it finds in the same configuration at the origin, with the same grid count"""
    _, ent = R.pose_map(3)
    move = R.shift(-1e5, 2e4)
    mstate = np.zeros(1, M.MSTATE)
    mstate["cur_slot"], mstate["cur_links"] = 1, 9
    curr = R.shift(12.0, -7.0)
    near = M.ref_select(mref, mstate, ent, curr, 32)
    moved = ent.copy()
    for j in range(3):
        moved[j]["h_origin_key"] = ent[j]["h_origin_key"] @ move
    far = M.ref_select(mref, mstate, moved, curr @ move, 32)
    assert near[0] >= 0 and near[1] >= 32 and far[:2] == near[:2] and np.abs(far[2] - near[2]).max() <= 1e-3
    assert M.np_select(mstate[0], moved, curr @ move, 32)[:2] == far[:2]


def test_too_far_and_singular_are_refused(rref, mref):
    eye = R.entries([np.eye(3)])
    too = R.shift(H.TOO_FAR, 0.0)
    assert R.ref_setup(rref, too, eye) is None and R.ref_setup(rref, np.eye(3), R.entries([too])) is None
    assert M.ref_relative(mref, np.eye(3), R.entries([too])[0]) is None and not M.np_invertible(too)
    assert R.ref_fit_view(rref, R.entries([too]), 320, 224, 0.0) is None
    # the limit is 320 x 10^4 px at unit scale
    assert R.ref_setup(rref, R.shift(3.1e6, 0.0), eye) is not None and R.ref_setup(rref, R.shift(3.3e6, 0.0), eye) is None
    # what the parent refused for a real reason still fails
    for bad in (np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]]), H.diag(1, 1e-13), H.diag(1, 1, 0)):
        assert R.ref_setup(rref, bad, eye) is None and R.ref_setup(rref, np.eye(3), R.entries([bad])) is None
        assert M.ref_relative(mref, np.eye(3), R.entries([bad])[0]) is None and not M.np_invertible(bad)


def test_minified_overview_far_from_a_corner(rref, mref):
    """a view of scale 0.1 with a translation of 4 000 px: det 0.01 was below 1e-12 x 4000^3"""
    v = np.array([[0.1, 0.0, 4000.0], [0.0, 0.1, 0.0], [0.0, 0.0, 1.0]])
    s = R.ref_setup(rref, v, R.entries([np.eye(3)]))
    want = np.linalg.inv(v)
    assert s is not None and _rel(s, want / want[2, 2]) <= 1e-9 and M.np_invertible(v)
    assert M.ref_relative(mref, np.eye(3), R.entries([v])[0]) is not None


def test_far_map_renders_as_at_the_origin(render):
    H.check_far(render)
