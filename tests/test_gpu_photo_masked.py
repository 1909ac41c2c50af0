"""The robust photometric alignment on the template pixels a mask admits, on the device (include/hnet.h hnet_op_photo_align_masked;
csrc/kernels_photo_masked.hip): a full mask against hnet_op_photo_align_robust byte for byte, every mask of photo_masked_util and the cover of
the two-keyframe composite against the host reference tests/cpp/photo_masked_ref.cpp, img1 under refused bytes, bitwise independence of the batch, the
composite rows against their CPU-fixed gates, and the refusals.  Calls of n = 1 .. 4.  Main model prior-3, N = 16, max_batch 8."""
import ctypes as C

import numpy as np
import pytest

import keyframe_localise_util as KL
import keyframe_render_util as KR
import photo_align_util as U
import photo_masked_util as M
import photo_robust_util as R

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = 1, 5
LEVELS, K = 4, 6
OFFSETS_VS_REFERENCE_PX = 1e-4          # final offsets, device against host reference: the bound of test_gpu_photo_robust.py


@pytest.fixture(scope="module")
def mref(tmp_path_factory):
    return M.build_ref(tmp_path_factory.mktemp("photo_masked_ref_gpu"))


@pytest.fixture(scope="module")
def render_ref(tmp_path_factory):
    return KR.build_ref(tmp_path_factory.mktemp("photo_masked_render_ref_gpu"))


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=8)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pair():
    i1, i2, _ = U.smooth_pair(1, 2.0)
    return i1, i2


def _against_reference(dev_out, dev_lv, ref_out, ref_lv, names):
    """every integer of every level equal, the offsets within 1e-4 px (bit for bit where the level made no trial), out = level 0"""
    for b, name in enumerate(names):
        assert dev_out[b].tobytes() == dev_lv[b, 0].tobytes(), name
        for L in range(dev_lv.shape[1]):
            d, r = dev_lv[b, L], ref_lv[b, L]
            assert M.trace(d) == M.trace(r), (name, L, M.trace(d), M.trace(r))
            diff = float(np.abs(d["px"]["offsets_px"].astype(np.float64) - r["px"]["offsets_px"]).max())
            assert diff <= OFFSETS_VS_REFERENCE_PX, (name, L, diff)
            if d["px"]["trials"] == 0:
                assert d["px"]["offsets_px"].tobytes() == r["px"]["offsets_px"].tobytes(), (name, L)
            if d["px"]["flags"] & U.FEW_PIXELS:
                assert not d["info10"].any() and not d["grad10"].any() and d["px"]["mse0"] == 0.0, (name, L)


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("n", [1, 3])
def test_full_mask_is_the_robust_call(eng, n, levels):
    """a mask without a zero byte (255 and other non-zero values) gives hnet_op_photo_align_robust's `out` and `levels_out` byte for byte: the order of
    every addition is the robust kernel's"""
    i1, i2, _, start = R.row_pairs("block-4levels")
    i1, i2, start = i1[:n], i2[:n], start[:n]
    mask = np.full_like(i1, 255)
    mask[:, ::3, ::5] = 1
    want, wlv = eng.op_photo_align_robust(i1, i2, start, levels=levels, want_levels=True, max_iterations=8)
    out, lv = eng.op_photo_align_masked(i1, mask, i2, start, levels=levels, want_levels=True, max_iterations=8)
    assert out.tobytes() == want.tobytes() and lv.tobytes() == wlv.tobytes()
    assert (lv["px"]["trials"] > 0).any() and (lv["n_outliers"] > 0).any()


@pytest.mark.parametrize("min_valid", [20000, M.SPARSE_MIN_VALID])
def test_masks_match_reference(eng, mref, render_ref, pair, min_valid):
    """one zero byte, one set byte per quad in each of the four positions, the last row and column alone, rows 0 - 95 zero (three whole slices return early
    at every level), a checkerboard (levels 1 - 3 empty: FEW_PIXELS; level 0 runs from the call's start), all zero and the cover of the two-keyframe
    composite, in calls of n = 4, 4 and 3 with the default min_valid and with 500 (so that the sparse masks run): every integer of every level equals the host
    reference's and the offsets lie within 1e-4 px"""
    i1, i2 = pair
    cases = dict(M.masks())
    cases["two-keyframe-cover"] = KL.composite(render_ref, "two-keyframes-drift8", 1)[1]
    names = list(cases)
    for lo in range(0, len(names), 4):
        grp = names[lo:lo + 4]
        masks = np.stack([cases[k] for k in grp])
        a, b, start = np.stack([i1] * len(grp)), np.stack([i2] * len(grp)), np.zeros((len(grp), 8), np.float32)
        out, lv = eng.op_photo_align_masked(a, masks, b, start, levels=LEVELS, want_levels=True, max_iterations=K, min_valid=min_valid)
        rout, rlv = M.ref_run(mref, a, masks, b, start, LEVELS, max_iterations=K, min_valid=min_valid)
        for j, name in enumerate(grp):
            print(f"{name}, min_valid {min_valid}: " + "; ".join(f"L{L} {M.trace(lv[j, L])}" for L in range(LEVELS - 1, -1, -1)))
        _against_reference(out, lv, rout, rlv, grp)
        for j, name in enumerate(grp):
            if name == "all-zero":
                assert (lv[j]["px"]["flags"] == U.FEW_PIXELS).all() and not lv[j]["px"]["n_valid0"].any()
            if name == "checkerboard":
                assert (lv[j, 1:]["px"]["flags"] == U.FEW_PIXELS).all() and not lv[j, 1:]["px"]["n_valid0"].any() and lv[j, 0]["px"]["trials"] > 0
            if name in ("rows-0-95-zero", "one-zero-byte", "two-keyframe-cover"):
                assert (lv[j]["px"]["trials"] > 0).all() and not (lv[j]["px"]["flags"] & U.FEW_PIXELS).any(), name
            if name.startswith("quad-byte") and min_valid == M.SPARSE_MIN_VALID:
                assert lv[j, 0]["px"]["trials"] > 0 and 15000 < lv[j, 0]["px"]["n_valid0"] <= 17920, name


def test_img1_under_refused_bytes_is_never_read(eng, pair):
    """img1 scrambled under the zero mask bytes gives equal bytes at every level (a coarse img1 pixel whose box mean mixes admitted and refused bytes is
    never used)"""
    i1, i2 = pair
    names = ["one-zero-byte", "quad-byte-2", "rows-0-95-zero", "checkerboard"]
    masks = np.stack([M.masks()[k] for k in names])
    clean, dirty = np.stack([i1] * 4), np.stack([M.scramble_under(i1, m) for m in masks])
    assert (clean != dirty).any(axis=(1, 2)).all()
    b, start = np.stack([i2] * 4), np.zeros((4, 8), np.float32)
    want = eng.op_photo_align_masked(clean, masks, b, start, levels=LEVELS, want_levels=True, max_iterations=K, min_valid=M.SPARSE_MIN_VALID)
    got = eng.op_photo_align_masked(dirty, masks, b, start, levels=LEVELS, want_levels=True, max_iterations=K, min_valid=M.SPARSE_MIN_VALID)
    assert want[0].tobytes() == got[0].tobytes() and want[1].tobytes() == got[1].tobytes()


def test_batch_independence(eng, pair):
    """a job alone, as slot 0 of 3 and as slot 2 of 3, twice, gives equal bytes, beside jobs whose masks are empty or return early in other slices"""
    i1, i2 = pair
    b1, b2, _, bs = R.row_pairs("block-4levels")
    ms = M.masks()
    job = (b1[2], ms["rows-0-95-zero"], b2[2], bs[2])
    others = [(i1, ms["all-zero"], i2, np.zeros(8, np.float32)), (i1, ms["checkerboard"], i2, np.zeros(8, np.float32))]

    def run(jobs):
        a, m, b, s = (np.stack([j[k] for j in jobs]) for k in range(4))
        return eng.op_photo_align_masked(a, m, b, s, levels=LEVELS, want_levels=True, max_iterations=K)
    alone = run([job])
    assert (alone[1]["px"]["trials"] > 0).all()
    for _ in range(2):
        first, last = run([job] + others), run(others + [job])
        assert first[0][0].tobytes() == alone[0][0].tobytes() and first[1][0].tobytes() == alone[1][0].tobytes()
        assert last[0][2].tobytes() == alone[0][0].tobytes() and last[1][2].tobytes() == alone[1][0].tobytes()
        assert run([job])[1].tobytes() == alone[1].tobytes()


@pytest.mark.parametrize("name", list(KL.ROWS))
def test_composite_rows_on_device(eng, mref, render_ref, name):
    """the composite rows of the CPU test on seeds 1, 2, 5, 11 in one call of n = 4: the device ends within 1e-4 px of the host reference with its integers
    at every level, within the row's CPU-fixed gate of the truth; on the two-keyframe rows the masked mean cost is below 10, hnet_op_photo_align_robust's
    on the same composite above 100 and further from the truth for every seed"""
    scenes = [KL.scene(name, seed) for seed in KL.SEEDS]
    comps = [KL.composite(render_ref, name, seed) for seed in KL.SEEDS]
    tmpl, cover, frames = np.stack([c[0] for c in comps]), np.stack([c[1] for c in comps]), np.stack([s["frame"] for s in scenes])
    start = np.zeros((4, 8), np.float32)
    out, lv = eng.op_photo_align_masked(tmpl, cover, frames, start, levels=KL.LEVELS, want_levels=True, max_iterations=KL.TRIALS)
    rout, rlv = M.ref_run(mref, tmpl, cover, frames, start, KL.LEVELS, max_iterations=KL.TRIALS)
    _against_reference(out, lv, rout, rlv, [f"{name}-{seed}" for seed in KL.SEEDS])
    plain = eng.op_photo_align_robust(tmpl, frames, start, levels=KL.LEVELS, max_iterations=KL.TRIALS)
    gate = KL.GATES[name]
    for i, seed in enumerate(KL.SEEDS):
        err, err_plain = KL.worst_corner_px(out[i]["px"]["offsets_px"], scenes[i]["truth"]), KL.worst_corner_px(plain[i]["px"]["offsets_px"], scenes[i]["truth"])
        print(f"{name} seed {seed}: masked {err:.4f} px (gate {gate:.4f}, mse {out[i]['px']['mse']:.2f}), existing alignment {err_plain:.4f} px "
              f"(mse {plain[i]['px']['mse']:.1f})")
        assert err < gate, (name, seed, err)
        if name.startswith("two-keyframes"):
            assert out[i]["px"]["mse"] < KL.MASKED_MSE_BELOW and plain[i]["px"]["mse"] > KL.UNMASKED_MSE_ABOVE and err < err_plain, (name, seed)
        else:
            assert out[i].tobytes() == plain[i].tobytes(), (name, seed)


def test_refusals_write_nothing(eng, pair):
    """what hnet_op_photo_align_robust refuses, and a NULL mask, return the documented code and leave `out` and `levels_out` untouched; a legal call writes
    its own records and nothing behind them"""
    from cuahn_vio_amd import _capi
    L = _capi.lib()
    size = _capi.PHOTO_ROBUST_DTYPE.itemsize
    i1, i2 = pair
    n_buf = 9
    out, lvo = np.full(n_buf * size, 0xA5, np.uint8), np.full(n_buf * 4 * size, 0x5A, np.uint8)
    keep, keep_lv = out.copy(), lvo.copy()
    a, b, m = np.ascontiguousarray(np.stack([i1] * n_buf)), np.ascontiguousarray(np.stack([i2] * n_buf)), np.full((n_buf, 224, 320), 255, np.uint8)
    x0 = np.zeros((n_buf, 8), np.float32)
    ok = _capi.photo_robust_opts()

    def call(n, o, levels=4, img1=a.ctypes.data, mask=m.ctypes.data, img2=b.ctypes.data, x=x0.ctypes.data, outp=out.ctypes.data):
        return L.hnet_op_photo_align_masked(eng.handle, img1, mask, img2, n, x, C.addressof(o) if o is not None else None, levels, outp, lvo.ctypes.data)
    assert call(1, ok, mask=None) == INVALID
    assert call(1, ok, levels=0) == INVALID and call(1, ok, levels=5) == INVALID and call(1, ok, levels=-1) == INVALID
    assert call(1, ok, outp=None) == INVALID and call(1, ok, img1=None) == INVALID and call(1, ok, img2=None) == INVALID and call(1, ok, x=None) == INVALID
    assert call(1, None) == INVALID and call(0, ok) == INVALID and call(-1, ok) == INVALID
    assert call(9, ok) == CAPACITY
    nan, inf = float("nan"), float("inf")
    for kw in (dict(max_iterations=33), dict(min_valid=-1), dict(lambda0=1.0000001e100), dict(eps_px=-1.0), dict(brightness=2), dict(brightness=-1),
               dict(huber_k=-1.0), dict(huber_k=nan), dict(huber_k=inf), dict(gain0=0.0), dict(gain0=-1.0), dict(gain0=nan), dict(gain0=inf),
               dict(bias0=nan), dict(bias0=-inf), dict(brightness=0, gain0=1.5), dict(brightness=0, bias0=-1.0)):
        assert call(1, _capi.photo_robust_opts(**kw)) == INVALID, kw
    assert out.tobytes() == keep.tobytes() and lvo.tobytes() == keep_lv.tobytes()
    assert call(1, _capi.photo_robust_opts(max_iterations=1), levels=4) == 0                                    # (a legal call does write both)
    assert out[:size].tobytes() != keep[:size].tobytes() and out[size:].tobytes() == keep[size:].tobytes()
    assert lvo[:4 * size].tobytes() != keep_lv[:4 * size].tobytes() and lvo[4 * size:].tobytes() == keep_lv[4 * size:].tobytes()
    assert eng.last_photo_align_device_ms() > 0.0
