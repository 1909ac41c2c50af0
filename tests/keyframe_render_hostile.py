"""What the CPU and the GPU tests of the keyframe render at hostile views share (include/hnet_keyframe_render.h, include/hnet_keyframe_map.h inverse;
DESIGN 7ac): a PLAIN reference of one entry in numpy float64 that does not read the header (positions, validity, a float64 bilinear blend), a restated
composite in numpy integers (the m-entry image, cover and counters from the one-entry renders), and the named cases: the counter widths, the tile
edges, the hostile views with the condition each must show on the reference, the hostile entries and the map far from the origin.
tests/test_keyframe_render_hostile_cpu.py checks every condition on the host reference (tests/cpp/keyframe_render_ref.cpp);
tests/test_gpu_keyframe_render_hostile.py checks them again and asserts the device equal to that reference byte for byte.  Nothing here is taken from the
device."""
import functools

import numpy as np

import keyframe_render_util as R

FEW, NEW, MEAN = R.MODES
H, W = R.H, R.W
BORDER_PX = 1e-9               # a plain position this close to the keyframe's border is not compared: the two inverses may fall on either side
EXCLUDED_MAX = 1e-3            # at most this share of a comparison view may be excluded so
BYTE_TOL = 0.5 + 1e-3          # |byte - plain|: the rounding to a byte, and about ten fp32 roundings of values up to 255 (1.5e-4) with room


def diag(a, b, c=1.0):
    return np.diag([float(a), float(b), float(c)])


def persp(gx, gy):
    return np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [gx, gy, 1.0]])


# ---- the plain reference of ONE entry: S = h_origin_key . inverse(view) by LAPACK, everything in float64

def plain_positions(h_origin_key, view, width, height):
    """-> (x, y, Z) [height, width] of every view pixel in the stored keyframe"""
    s = np.asarray(h_origin_key, np.float64).reshape(3, 3) @ np.linalg.inv(np.asarray(view, np.float64).reshape(3, 3))
    v, u = np.mgrid[0:height, 0:width].astype(np.float64)
    with np.errstate(all="ignore"):
        X, Y, Z = (s[i, 0] * u + s[i, 1] * v + s[i, 2] for i in range(3))
        return X / Z, Y / Z, Z


def plain_render(image, h_origin_key, view, width, height):
    """-> (value f64 [height, width] (0 where not valid), valid bool, near bool: within BORDER_PX of the keyframe's border)"""
    x, y, Z = plain_positions(h_origin_key, view, width, height)
    with np.errstate(all="ignore"):
        valid = (Z > 0) & (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
        near = np.minimum(np.minimum(np.abs(x), np.abs(x - (W - 1))), np.minimum(np.abs(y), np.abs(y - (H - 1)))) <= BORDER_PX
    xs, ys = np.where(valid, x, 0.0), np.where(valid, y, 0.0)
    x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = xs - x0, ys - y0
    img = np.asarray(image, np.float64).reshape(H, W)
    top = img[y0, x0] * (1 - fx) + img[y0, x1] * fx
    bot = img[y1, x0] * (1 - fx) + img[y1, x1] * fx
    return np.where(valid, top * (1 - fy) + bot * fy, 0.0), valid, near


def check_plain(out, cover, image, h_origin_key, view, width, height):
    """a one-entry render against the plain reference -> (excluded share, largest |byte - plain| where both cover): the cover equals the plain validity
    at every pixel that is not excluded, at most EXCLUDED_MAX of the view is excluded, and the bytes lie within BYTE_TOL"""
    val, valid, near = plain_render(image, h_origin_key, view, width, height)
    assert cover.max() <= 1
    wrong = ((cover == 1) != valid) & ~near
    share = float(near.sum()) / (width * height)
    both = (cover == 1) & valid
    worst = float(np.abs(out[both].astype(np.float64) - val[both]).max()) if both.any() else 0.0
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:4])
    assert share <= EXCLUDED_MAX, share
    assert worst <= BYTE_TOL, worst
    return share, worst


# ---- the restated composite, in integers: the m-entry render from the one-entry renders

def composite(imgs, covers, links, serials, mode):
    """imgs, covers [m, h, w] (cover 0 / 1) of the one-entry renders, the entries' links and serials -> (image, cover, n_covered, n_overlap, n [8], sse [8]):
    FEWEST_LINKS = argmin links then the lower slot, NEWEST = argmax serial then the lower slot, MEAN = (sum + cover // 2) // cover"""
    v, c = np.asarray(imgs).astype(np.int64), np.asarray(covers).astype(np.int64)
    m = v.shape[0]
    assert c.max() <= 1
    cover = c.sum(axis=0)
    slot = np.arange(m).reshape(m, 1, 1)
    big = np.int64(1) << 40
    if mode == MEAN:
        out = ((v * c).sum(axis=0) + cover // 2) // np.maximum(cover, 1)
    else:
        rank = np.asarray(links, np.int64).reshape(m, 1, 1) if mode == FEW else -np.asarray(serials, np.int64).reshape(m, 1, 1)
        key = np.where(c == 1, rank * 16 + slot, big)                              # (|rank| < 2^31: the slot breaks the ties, an uncovering entry never wins)
        out = np.take_along_axis(v, key.argmin(axis=0)[None], axis=0)[0]
    out = np.where(cover >= 1, out, 0)
    n, sse = np.zeros(8, np.uint64), np.zeros(8, np.uint64)
    seam = cover >= 2
    for j in range(m):
        on = seam & (c[j] == 1)
        n[j] = int(on.sum())
        sse[j] = int(((v[j][on] - out[on]) ** 2).sum())
    return out.astype(np.uint8), cover.astype(np.uint8), int((cover >= 1).sum()), int(seam.sum()), n, sse


def check_composite(render, images, ent, view, width, height):
    """render(images, entries, view, width, height, mode) -> (image, cover, record): the m-entry render equals the composite of that render's own
    one-entry renders, byte for byte, in the three modes"""
    m = len(ent)
    for mode in R.MODES:
        ones = [render(images[j:j + 1], ent[j:j + 1], view, width, height, mode) for j in range(m)]
        img, cover, n_cov, n_ov, n, sse = composite([o[0] for o in ones], [o[1] for o in ones], ent["links"], ent["serial"], mode)
        got, gcover, rec = render(images, ent, view, width, height, mode)
        r = rec[0]
        assert got.tobytes() == img.tobytes() and gcover.tobytes() == cover.tobytes(), (m, mode)
        assert (int(r["n_covered"]), int(r["n_overlap"])) == (n_cov, n_ov) and r["n"].tolist() == n.tolist() and r["sse"].tolist() == sse.tolist(), (m, mode, r, n, sse)


@functools.lru_cache(maxsize=None)
def tie_map():
    """pose_map(3) with equal links and equal serials: the tie rule (the lower slot) decides FEWEST_LINKS and NEWEST"""
    images, ent = R.pose_map(3)
    e = ent.copy()
    e["links"], e["serial"] = 2, 5
    e.setflags(write=False)
    return images, e


# the views compared with the plain reference: name -> (view, width, height, the entries of pose_map(3) rendered alone).  Generic, so that the plain
# reference alone excludes next to nothing: an axis-aligned view puts whole rows of positions ON the border.  Under the strong perspective entry 0, the
# identity, is left out for that reason: x = u / Z and y = v / Z put row 0 and column 0 on the border, 0.76 % of the view
STRONG = persp(0.02, 0.03)
PLAIN_VIEWS = {
    "turned": (R.view(320, 224), 320, 224, (0, 1, 2)),
    "scaled": (R.view(50, 37), 50, 37, (0, 1, 2)),
    "strong-perspective": (STRONG, 320, 224, (1, 2)),
}


# ---- 1. the width of the counters: closed forms

@functools.lru_cache(maxsize=None)
def flat_map(m):
    """m identity entries whose images alternate 0 and 255; links j and serial j + 1: FEWEST_LINKS shows slot 0, NEWEST the last"""
    images = np.zeros((m, H, W), np.uint8)
    images[1::2] = 255
    e = R.entries([np.eye(3)] * m)
    images.setflags(write=False)
    e.setflags(write=False)
    return images, e


def _vec(pairs):
    a = [0] * 8
    for j, x in pairs:
        a[j] = x
    return a


SSE_FULL = 255 * 255 * H * W                         # 4 660 992 000 > 2^32
assert SSE_FULL == 4660992000 and SSE_FULL > 1 << 32
# name -> (m, view, width, height, mode, n_covered, n_overlap, n [8], sse [8]); every view pixel is covered by every entry
COUNTER_CASES = {
    "two-flat-fewest": (2, np.eye(3), 320, 224, FEW, 71680, 71680, _vec([(0, 71680), (1, 71680)]), _vec([(1, SSE_FULL)])),
    "two-flat-newest": (2, np.eye(3), 320, 224, NEW, 71680, 71680, _vec([(0, 71680), (1, 71680)]), _vec([(0, SSE_FULL)])),
    # the mean of 0 and 255 is (255 + 1) // 2 = 128
    "two-flat-mean": (2, np.eye(3), 320, 224, MEAN, 71680, 71680, _vec([(0, 71680), (1, 71680)]), _vec([(0, 128 * 128 * 71680), (1, 127 * 127 * 71680)])),
    # 1024 x 512 pixels at a quarter of a keyframe pixel each: 524 288 x 255^2 = 34 091 827 200 in every odd slot
    "eight-flat-1024x512": (8, diag(4, 4), 1024, 512, FEW, 524288, 524288, [524288] * 8, _vec([(j, 34091827200) for j in (1, 3, 5, 7)])),
    # ONE full tile of one workgroup: 1024 pixels x 255^2 = 66 585 600 per counter, the bound of the kernel's header comment (< 2^32)
    "eight-flat-one-tile": (8, np.eye(3), 64, 16, FEW, 1024, 1024, [1024] * 8, _vec([(j, 1024 * 65025) for j in (1, 3, 5, 7)])),
}
assert 524288 * 65025 == 34091827200 and 1024 * 65025 < 1 << 32


# ---- 2. the edges of the 64 x 16 tile, and the largest views

TILE_SIZES = [(w, h) for w in (63, 64, 65, 127, 129) for h in (15, 16, 17, 33)] + [(8192, 1), (1, 8192), (8192, 17), (17, 8192)]
GUARD_SIZES = [(65, 17), (127, 33), (8192, 1), (17, 8192)]         # those called through raw ctypes with guarded output buffers
GUARD_BYTES, GUARD_FILL = 256, 0xA5


def tile_view(width, height):
    """the origin frame scaled into the view (pixel areas onto pixel areas; a one-pixel side keeps an inverse)"""
    return diag(width / 320.0, height / 224.0)


# ---- 3. the hostile views.  name -> (view, width, height).  Each is rendered with identity_first(), in the three modes

@functools.lru_cache(maxsize=None)
def identity_first():
    """pose_map(3) with entry 0's h_origin_key exactly the identity"""
    images, ent = R.pose_map(3)
    e = ent.copy()
    e[0]["h_origin_key"] = np.eye(3)
    e.setflags(write=False)
    return images, e


DENORMAL = np.eye(3)
DENORMAL[2, 0] = 5e-324
VIEWS = {
    "horizon": (persp(1 / 160.0, 0.0), 320, 224),
    "mirror": (R.shift(319.0, 0.0) @ diag(-1, 1), 320, 224),
    "quarter-turn": (np.array([[0.0, -1.0, 223.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), 224, 320),
    "half-turn-unshifted": (diag(-1, -1), 320, 224),
    "half-turn": (R.shift(319.0, 223.0) @ diag(-1, -1), 320, 224),
    "negative-8": (diag(1, 1, -1), 320, 224),                  # the composed [8] is negative: renormalised, S = diag(-1, -1, 1) like the unshifted half turn
    "strong-perspective": (STRONG, 320, 224),
    "minify-1e-3": (diag(1e-3, 1e-3), 65, 17),
    "magnify-1e3": (diag(1e3, 1e3) @ R.shift(-100.3, -80.7), 130, 33),
    "near-singular-accepted": (diag(1, 1e-5), 320, 224),
    "near-singular-refused": (diag(1, 1e-13), 320, 224),
    "scaled-1e-3": (1e-3 * np.eye(3), 320, 224),
    "overflow-1e150": (1e150 * np.eye(3), 320, 224),
    "vanish-1e-150": (1e-150 * np.eye(3), 320, 224),
    "denormal-in-6": (DENORMAL, 320, 224),
}
REFUSED_VIEWS = ("near-singular-refused", "overflow-1e150", "vanish-1e-150")          # the rule skips every entry under these
LIKE_IDENTITY = ("scaled-1e-3", "denormal-in-6")                                      # these render what the identity view renders
# a one-entry identity map under these views returns the stored image so transformed
EXACT_IMAGES = {
    "mirror": lambda img: img[:, ::-1],
    "quarter-turn": lambda img: np.rot90(img, -1),             # view pixel (u, v) shows origin pixel (v, 223 - u)
    "half-turn": lambda img: img[::-1, ::-1],
}


def beyond_view(rec):
    """the bytes of a record after its h_origin_view: counters and masks"""
    return np.ascontiguousarray(rec).view(np.uint8).reshape(-1)[72:R.REC.itemsize].tobytes()


def zero_record(view, skipped):
    want = np.zeros(1, R.REC)
    want["h_origin_view"], want["skipped_mask"] = np.asarray(view, np.float64).reshape(3, 3), skipped
    return want


def check_view(name, render):
    """the condition of the table in DESIGN 7ac that shows the case is what its name says, on any render(images, entries, view, width, height, mode);
    -> {mode: (image, cover, record)} of identity_first() under the view"""
    view, w, h = VIEWS[name]
    images, ent = identity_first()
    got = {mode: render(images, ent, view, w, h, mode) for mode in R.MODES}
    one = lambda v=view, ww=w, hh=h: render(images[2:3], R.entries([np.eye(3)]), v, ww, hh, FEW)          # noqa: E731  (a one-entry identity map)
    for mode, (img, cover, rec) in got.items():
        r = rec[0]
        assert r["h_origin_view"].tobytes() == np.ascontiguousarray(view, np.float64).tobytes()
        assert r["used_mask"] | r["skipped_mask"] == 7 and r["used_mask"] & r["skipped_mask"] == 0
        assert r["n_covered"] == (cover >= 1).sum() and r["n_overlap"] == (cover >= 2).sum() and not img[cover == 0].any()
        if name in REFUSED_VIEWS:
            assert not img.any() and not cover.any() and rec.tobytes() == zero_record(view, 7).tobytes()
            continue
        assert r["used_mask"] == 7, (name, r)
        if name == "horizon":
            assert 0 < r["n_covered"] < w * h and not cover[:, 160:].any() and cover[:, :160].any()
        elif name == "strong-perspective":
            assert 0 < r["n_covered"] < 0.02 * w * h
        elif name == "minify-1e-3":
            assert r["n_covered"] == 1
        elif name == "magnify-1e3":
            assert r["n_covered"] == w * h
            for e in ent:                                                            # at most 4 texel neighbourhoods per entry
                x, y, _ = plain_positions(e["h_origin_key"], view, w, h)
                assert len(set(zip(np.floor(x).ravel().tolist(), np.floor(y).ravel().tolist()))) <= 4
        elif name in LIKE_IDENTITY:
            img_i, cover_i, rec_i = render(images, ent, np.eye(3), w, h, mode)
            assert img.tobytes() == img_i.tobytes() and cover.tobytes() == cover_i.tobytes() and r["n_overlap"] > 10000
            assert beyond_view(rec) == beyond_view(rec_i)       # (all but the view)
    if name == "horizon":
        # column 160 is where the identity entry's Z is EXACTLY 0
        _, _, Z = plain_positions(np.eye(3), view, w, h)
        assert (Z[:, 160] == 0.0).all() and (Z[:, :160] > 0).all() and (Z[:, 161:] < 0).all()
    if name in EXACT_IMAGES:
        img, cover, rec = one()
        assert img.tobytes() == np.ascontiguousarray(EXACT_IMAGES[name](images[2])).tobytes() and (cover == 1).all()
    if name in ("half-turn-unshifted", "negative-8"):
        img, cover, rec = one()
        want = np.zeros((h, w), np.uint8)
        want[0, 0] = 1
        assert cover.tobytes() == want.tobytes() and img[0, 0] == images[2][0, 0]
    return got


# ---- the same matrices as h_origin_key of entry 1 of pose_map(3), between two good entries

ENTRY_SLOT = 1
REFUSED_ENTRIES = ("near-singular-refused", "overflow-1e150", "vanish-1e-150")


def hostile_entries(name):
    images, ent = R.pose_map(3)
    e = ent.copy()
    e[ENTRY_SLOT]["h_origin_key"] = VIEWS[name][0]
    return images, e


def check_entry(name, render):
    """a refused matrix in one entry: only that bit moves to skipped_mask, and image, cover and the two pixel counters are those of the other entries'
    render; -> {mode: (image, cover, record)} under the turned 320 x 224 view"""
    images, e = hostile_entries(name)
    view, w, h, _ = PLAIN_VIEWS["turned"]
    others = [j for j in range(3) if j != ENTRY_SLOT]
    got = {mode: render(images, e, view, w, h, mode) for mode in R.MODES}
    for mode, (img, cover, rec) in got.items():
        r = rec[0]
        if name not in REFUSED_ENTRIES:
            assert (r["used_mask"], r["skipped_mask"]) == (7, 0), (name, r)
            continue
        assert (r["used_mask"], r["skipped_mask"]) == (7 & ~(1 << ENTRY_SLOT), 1 << ENTRY_SLOT), (name, r)
        img2, cover2, rec2 = render(images[others], e[others], view, w, h, mode)
        assert img.tobytes() == img2.tobytes() and cover.tobytes() == cover2.tobytes()
        assert (r["n_covered"], r["n_overlap"]) == (rec2[0]["n_covered"], rec2[0]["n_overlap"]) and r["n_overlap"] > 10000
        assert r["n"][others].tolist() == rec2[0]["n"][:2].tolist() and r["sse"][others].tolist() == rec2[0]["sse"][:2].tolist() and r["n"][ENTRY_SLOT] == 0
    return got


# ---- 5. far from the origin

FAR_SHIFT = (-1e5, 2e4)
FAR_T = (1e3, 9.9e3, 1.01e4, 1e5, 1e6)             # px; the parent refused everything beyond 10^4
TOO_FAR = 1e8                                      # beyond 320 x 10^4 px: still refused


@functools.lru_cache(maxsize=None)
def far_map():
    """-> (images, entries of pose_map(3) each right-multiplied by shift(FAR_SHIFT), the turned view moved the same way): the camera's origin is
    100 000 px from where the map was flown, every h_origin_key is as well conditioned as before"""
    images, ent = R.pose_map(3)
    move = R.shift(*FAR_SHIFT)
    e = ent.copy()
    for j in range(len(e)):
        e[j]["h_origin_key"] = ent[j]["h_origin_key"] @ move
    e.setflags(write=False)
    return images, e, R.view(320, 224) @ move


def check_far(render):
    """the moved map under the moved view renders the unmoved map under the unmoved view byte for byte; -> {mode: (image, cover, record)}"""
    images, e, view = far_map()
    _, ent = R.pose_map(3)
    got = {mode: render(images, e, view, 320, 224, mode) for mode in R.MODES}
    for mode, (img, cover, rec) in got.items():
        img0, cover0, rec0 = render(images, ent, R.view(320, 224), 320, 224, mode)
        assert (rec[0]["used_mask"], rec[0]["skipped_mask"]) == (7, 0), rec
        assert img.tobytes() == img0.tobytes() and cover.tobytes() == cover0.tobytes()
        assert beyond_view(rec) == beyond_view(rec0) and rec[0]["n_overlap"] > 10000
    return got
