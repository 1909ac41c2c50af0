"""What the CPU and the GPU tests of the three search stages at the edges of their shift domain share (include/hnet.h hnet_op_photo_search,
hnet_op_photo_search_oriented, hnet_op_photo_search_fine; csrc/kernels_photo_search*.hip): the cases.  Every case is a pair of level-2
thumbnails [56, 80] u8 that photo_search_fine_util.expand4 turns into frames of constant 4 x 4 blocks, so that the level-2 thumbnail and its level-3
reduction are exact, with its search options, its coarse table, its fine options and its fine table.  The pairs are cut from one seeded canvas the way
photo_search_util.hostile() cuts them, at level 2: image(u + sx, v + sy) = template(u, v).

Group 1: the nine sign combinations of the coarse corners and edges, at the even level-2 offset and at an odd one.  Group 2: min_overlap equal to the
overlap of a chosen shift, and one above.  Group 3: canvases at the ends of the number range.  Group 4: one pixel in a constant template, so that a shift
is scored exactly where its overlap holds the pixel.  Group 5: eight pairs of four kinds in one call.  tests/test_photo_search_hostile_cpu.py checks
every stated condition on the host reference; nothing here is taken from the device."""
import collections
import functools

import numpy as np

import photo_search_fine_util as F
import photo_search_oriented_util as O
import photo_search_util as S
from cuahn_vio_amd import _capi

FW, FH, TW, TH = F.FW, F.FH, S.TW, S.TH
MAX_SX, MAX_SY = 64, 44                    # the level-2 shift domain: 2 * 30 + 4, 2 * 20 + 4
SEED = 20261
QNAN64 = 0x7FF8000000000000                # hnet_search::quiet_nan_d

# a: the template as the coarse call sees it; turn: the oriented and the fine call see it point-mirrored, so that the half turn (entry 1) wins;
# calls: which of "coarse", "oriented", "fine" run on the pair; want: what the CPU test asserts of the reference (the keys are read there)
Case = collections.namedtuple("Case", "a b turn o entries fkw rows calls want")
ALL = ("coarse", "oriented", "fine")

IDENT = ((0.0, 1.0),)
HALF_TURN = ((0.0, 1.0), (180.0, 1.0))     # a half turn is exact in the integer warp: ix = 79 - u, fx = 0
# the fine rows of HALF_TURN: each holds its coarse entry's matrix twice and one other entry
ROWS_TWICE = (((0.0, 1.0), (10.0, 1.0), (0.0, 1.0)), ((10.0, 1.0), (180.0, 1.0), (180.0, 1.0)))
FINE3 = dict(radius=4, n_fine=3)
FINE1 = dict(radius=4, n_fine=1)
COARSE_TRUTHS = tuple((dx, dy) for dy in (-20, 0, 20) for dx in (-30, 0, 30))


@functools.lru_cache(maxsize=None)
def canvas(seed=SEED, smooth=2, lo=0, hi=255):
    """[56 + 2 * 44, 80 + 2 * 64] u8: uniform noise, `smooth` times under a 3 x 3 box and stretched to 0 .. 255; smooth = 0: noise of the two values lo, hi"""
    rng = np.random.RandomState(seed)
    h, w = FH + 2 * MAX_SY, FW + 2 * MAX_SX
    if not smooth:
        return np.where(rng.randint(0, 2, size=(h, w)) == 1, hi, lo).astype(np.uint8)
    t = rng.randint(0, 256, size=(h, w)).astype(np.int64)
    for _ in range(smooth):
        p = np.pad(t, 1, mode="edge")
        t = sum(p[i:i + h, j:j + w] for i in range(3) for j in range(3))
    return ((t - t.min()) * 255 // (t.max() - t.min())).astype(np.uint8)


def cut(cv, sx, sy):
    """image(u + sx, v + sy) = cut(cv, 0, 0)(u, v)"""
    assert abs(sx) <= MAX_SX and abs(sy) <= MAX_SY
    return np.ascontiguousarray(cv[MAX_SY - sy:MAX_SY - sy + FH, MAX_SX - sx:MAX_SX - sx + FW])


def down2(t):
    """the level-3 reduction of a level-2 thumbnail"""
    t = np.asarray(t, np.int64)
    return ((t[0::2, 0::2] + t[0::2, 1::2] + t[1::2, 0::2] + t[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def template(c, call):
    """the level-2 template the call `call` gets"""
    return np.ascontiguousarray(c.a[::-1, ::-1]) if c.turn and call != "coarse" else c.a


def frames(c, call):
    return F.expand4(template(c, call)), F.expand4(c.b)


def tables(lib, c):
    """-> (coarse table [n_hyp], fine options, fine table [n_hyp, n_fine]) of a case"""
    return O.table(lib, *c.entries), F.fine_opts(lib, **c.fkw), F.fine_rows(lib, *c.rows)


# ---- group 1: corners and edges of the domain

@functools.lru_cache(maxsize=None)
def corners():
    """name -> Case: the nine coarse truths at the level-2 offsets (2 dx, 2 dy) and (2 dx + 1, 2 dy - 1); of each truth's two pairs one is turned.  At the
    odd offset the level-3 thumbnails lie half a pixel apart: the coarse winner is one of the two nearest shifts on each axis, scores 0.70 .. 0.85 on the
    smoothed canvas (min_score 0.5), and the fine stage finds the exact offset from either."""
    cv, out = canvas(), {}
    a = cut(cv, 0, 0)
    for k, (dx, dy) in enumerate(COARSE_TRUTHS):
        for odd in (0, 1):
            sx, sy = 2 * dx + odd, 2 * dy - odd
            turn = (k + odd) % 2 == 1
            o = S.search_opts(min_overlap=16, min_score=0.5) if odd else S.search_opts(min_overlap=16)
            want = dict(coarse=None if odd else (dx, dy), fine=(sx, sy), hyp=int(turn), j=1 if turn else 0)
            out[f"{'odd' if odd else 'even'}({dx},{dy})"] = Case(a, cut(cv, sx, sy), turn, o, HALF_TURN, FINE3, ROWS_TWICE, ALL, want)
    return out


def batches(cases, size=8):
    """the names of `cases` in calls of up to `size` pairs that share options and tables"""
    groups = {}
    for name, c in cases.items():
        groups.setdefault((bytes(c.o), c.entries, tuple(sorted(c.fkw.items())), c.rows, c.calls), []).append(name)
    return [tuple(names[i:i + size]) for names in groups.values() for i in range(0, len(names), size)]


# ---- group 2: the overlap threshold at equality

def _paste(img, patch, sx, sy):
    """img with patch moved by (sx, sy) >= 0 pasted over it"""
    out = img.copy()
    h, w = out.shape
    out[sy:, sx:] = patch[:h - sy, :w - sx]
    return out


def thresholds(lib):
    """name -> (Case at min_overlap 16, the call, the chosen shift as an index into that call's score table of pair 0).  The CPU and the GPU test read the
    shift's n from the reference and run the case again at the two thresholds (with_min_overlap).
    coarse: the corner (30, 20), 10 x 8 pixels.  oriented: the template warped under (30 degrees, scale 0.8) sits in the image moved by (18, 10); the
    mask is ragged.  fine: the corner (64, 44), 16 x 12 pixels, and a shift at ex = 4 under a 45 degree entry."""
    cv = canvas()
    a = cut(cv, 0, 0)
    o16 = S.search_opts(min_overlap=16)
    out = {"coarse": (Case(a, cut(cv, 60, 40), False, o16, IDENT, FINE1, (IDENT,), ("coarse",), {}), "coarse", (40, 60))}
    ent = ((0.0, 1.0), (30.0, 0.8))
    t3 = cut(canvas(SEED + 1, smooth=1), 0, 0)[:TH, :TW]
    w3, _ = O.np_warp(t3, O.hyp(lib, *ent[1])["b"][0])
    b3 = _paste(cut(canvas(SEED + 2, smooth=1), 0, 0)[:TH, :TW], w3, 18, 10)
    up = lambda t: np.repeat(np.repeat(t, 2, axis=0), 2, axis=1)       # constant 2 x 2 blocks: the level-3 reduction is t
    out["oriented"] = (Case(up(t3), up(b3), False, o16, ent, FINE1, (IDENT, IDENT), ("oriented",), {}), "oriented", (1, 10 + S.RY, 18 + S.RX))
    out["fine"] = (Case(a, cut(cv, 60, 40), False, o16, IDENT, FINE1, (IDENT,), ("fine",), {}), "fine", (0, 8, 8))
    ent = ((0.0, 1.0), (45.0, 1.0))
    w2, _ = F.np_warp(a, O.hyp(lib, *ent[1])["b"][0])
    b2 = _paste(cut(canvas(SEED + 3), 0, 0), w2, 28, 16)
    out["fine-45"] = (Case(a, b2, False, S.search_opts(min_overlap=16, min_score=0.5), ent, FINE1, (IDENT, (ent[1],)), ("fine",), {}), "fine", None)
    return out


def with_min_overlap(c, min_overlap):
    kw = S.search_kw(c.o)
    kw["min_overlap"] = int(min_overlap)
    return c._replace(o=S.search_opts(**kw))


def fine_45_shift(lib, c):
    """the shift of the fine-45 case: the first (ex = 4, ey) whose masked n is a multiple of 4 -> ((j, ey + 4, ex + 4), n), n from the reference's sums"""
    w, m = F.ref_warp(lib, c.a, tables(lib, c)[2]["b"][1, 0])
    for ey in range(-4, 5):
        n = int(F.ref_shift(lib, w, m, c.b, 28 + 4, 16 + ey, 16)[0][0])
        if n % 4 == 0:
            return (0, ey + 4, 8), n
    raise AssertionError("no shift at ex = 4 has a masked overlap that is a multiple of 4")


THRESHOLDS = ("coarse", "oriented", "fine", "fine-45")


def threshold_runs(lib, name):
    """-> (the case with the threshold at the chosen shift's n, the case with the next threshold above, the call, the shift's index in pair 0's score table,
    n).  n is the host reference's: the winner's n_overlap of the coarse and the oriented call, the sums of the shift for the fine ones, whose threshold is
    4 * min_overlap: the nearest pair that brackets n, equal to n where n is a multiple of 4."""
    c, call, idx = thresholds(lib)[name]
    a, b = frames(c, call)
    if name == "coarse":
        rec, _ = S.ref_run(lib, a[None], b[None], c.o)
        assert (rec["dx"][0], rec["dy"][0]) == (30, 20)
        n, per = int(rec["n_overlap"][0]), 1
    elif name == "oriented":
        rec, _ = O.ref_run(lib, a[None], b[None], c.o, tables(lib, c)[0])
        assert (rec["hyp"][0], rec["base"]["dx"][0], rec["base"]["dy"][0]) == (1, 18, 10)
        n, per = int(rec["base"]["n_overlap"][0]), 1
    elif name == "fine":
        n, per = int(F.ref_shift(lib, c.a, np.ones_like(c.a), c.b, MAX_SX, MAX_SY, 16)[0][0]), 4
    else:
        (idx, n), per = fine_45_shift(lib, c), 4
    return with_min_overlap(c, n // per), with_min_overlap(c, n // per + 1), call, idx, n


# ---- group 3: the number range

@functools.lru_cache(maxsize=None)
def number_range():
    """name -> Case: canvases of {254, 255}, {0, 1} and {0, 255} at the truths (0, 0), (30, 20) and (-30, -20), and a template of all 255 under a 45 degree
    entry.  A constant template has no variance under any mask, so that last pair is NO_TEXTURE in the coarse stage and the fine stage is SKIPPED."""
    out = {}
    for kind, lo, hi in (("bright", 254, 255), ("dark", 0, 1), ("extreme", 0, 255)):
        cv = canvas(SEED + 10 + lo, smooth=0, lo=lo, hi=hi)
        for dx, dy in ((0, 0), (30, 20), (-30, -20)):
            want = dict(coarse=(dx, dy), fine=(2 * dx, 2 * dy), hyp=0, j=0)
            out[f"{kind}({dx},{dy})"] = Case(cut(cv, 0, 0), cut(cv, 2 * dx, 2 * dy), False, S.search_opts(min_overlap=16), IDENT, FINE3, ROWS_TWICE[:1], ALL, want)
    ent = ((0.0, 1.0), (45.0, 1.0))
    out["all-255-under-45"] = Case(np.full((FH, FW), 255, np.uint8), cut(canvas(), 0, 0), False, S.search_opts(min_overlap=16), ent, FINE1, ((ent[1],), (ent[1],)), ALL,
                                   dict(skipped=True))
    # what does reach the fine kernel under the ragged 45 degree mask with every byte at 254 or 255: the coarse stage finds the pair under the identity,
    # whose fine row holds the 45 degree entry alone; the fine score is low, the sums are near their largest
    a = out["bright(0,0)"].a
    out["bright-under-45"] = Case(a, a, False, S.search_opts(min_overlap=16), IDENT, FINE1, ((ent[1],),), ("fine",), dict(coarse=(0, 0), hyp=0, masked=True))
    return out


# ---- group 4: exact zero variance inside a scored table

# (u, v) of the template's pixel, the level-2 move of the image: the corners and both sides of a dword boundary at both ends of a middle row, the image
# the same thumbnail.  Within |ex| <= 4 the overlap never loses column 4 or 75, so those two also come with the image moved by 4 columns (its pixel in
# column 0 or 79), where the fine table is mixed as well.
PIXELS = (((0, 0), 0), ((79, 0), 0), ((0, 55), 0), ((79, 55), 0), ((3, 28), 0), ((4, 28), 0), ((75, 28), 0), ((76, 28), 0), ((4, 28), -4), ((75, 28), 4))


@functools.lru_cache(maxsize=None)
def single_pixels():
    """name -> Case: a template of 77 with one pixel of 200, the image the same thumbnail (moved by `move` columns).  A shift is scored exactly where its
    overlap holds the template's pixel on the template's side and the image's pixel on the image's: elsewhere a variance is exactly 0."""
    out = {}
    for (u, v), move in PIXELS:
        t, b = np.full((FH, FW), 77, np.uint8), np.full((FH, FW), 77, np.uint8)
        t[v, u], b[v, u + move] = 200, 200
        want = dict(coarse=(move // 2, 0), fine=(move, 0), hyp=0, j=0, pixel=(u, v), image_pixel=(u + move, v))
        out[f"pixel({u},{v}){move:+d}" if move else f"pixel({u},{v})"] = Case(t, b, False, S.search_opts(min_overlap=16), IDENT, FINE1, (IDENT,), ("coarse", "fine"), want)
    return out


def holds(w, h, pt, pi, sx, sy):
    """whether the overlap of shift (sx, sy) of a w x h thumbnail holds pixel pt on the template's side and pixel pi on the image's"""
    u0, u1, v0, v1 = max(0, -sx), min(w, w - sx), max(0, -sy), min(h, h - sy)
    return u0 <= pt[0] < u1 and v0 <= pt[1] < v1 and u0 + sx <= pi[0] < u1 + sx and v0 + sy <= pi[1] < v1 + sy


# ---- group 5: neighbours in one call

NEIGHBOUR_KINDS = ("refined", "skipped", "nothing", "low", "refined", "skipped", "nothing", "refined")
# entry 1's row holds scale-0.5 entries: their masks (columns 20 .. 59, rows 14 .. 41) meet the overlap of a corner shift in at most 24 < 4 * 16 pixels
ROWS_NEIGHBOURS = (ROWS_TWICE[0], ((180.0, 0.5), (170.0, 0.5), (180.0, 0.5)))


@functools.lru_cache(maxsize=None)
def neighbours():
    """-> the 8 Cases of one call under one set of options (fine min_score 1.0) and tables: corner pairs that are REFINED with score exactly 1.0; unrelated
    images (coarse LOW_SCORE, fine SKIPPED); turned corner pairs whose winner, entry 1, has the scale-0.5 row (NOTHING_SCORED); a pair whose image
    differs from the template in the last bit of 40 pixels (LOW_SCORE below 1.0)"""
    cv, other = canvas(), canvas(SEED + 30)
    a = cut(cv, 0, 0)
    near = a.copy()
    near[10:14, 20:30] ^= 1
    o, fkw = S.search_opts(min_overlap=16), dict(radius=4, n_fine=3, min_score=1.0)
    corner = iter(((30, 20), (-30, 20), (30, -20)))
    nothing = iter(((-30, -20), (30, -20)))
    far = iter(((7, 3), (-20, 11)))
    out = []
    for kind in NEIGHBOUR_KINDS:
        if kind == "refined":
            dx, dy = next(corner)
            b, turn, want = cut(cv, 2 * dx, 2 * dy), False, dict(flags=_capi.PSF_REFINED, coarse=(dx, dy), fine=(2 * dx, 2 * dy), hyp=0, j=0)
        elif kind == "nothing":
            dx, dy = next(nothing)
            b, turn, want = cut(cv, 2 * dx, 2 * dy), True, dict(flags=_capi.PSF_NOTHING_SCORED, coarse=(dx, dy), hyp=1)
        elif kind == "low":
            b, turn, want = near, False, dict(flags=_capi.PSF_LOW_SCORE, coarse=(0, 0), hyp=0)
        else:
            b, turn, want = cut(other, *next(far)), False, dict(flags=_capi.PSF_SKIPPED)
        out.append(Case(a, b, turn, o, HALF_TURN, fkw, ROWS_NEIGHBOURS, ("fine",), want))
    return tuple(out)
