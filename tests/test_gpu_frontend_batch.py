"""The image front end (csrc/kernels.hip prep_* / warp_* / errmap_kernel, warp_dev.h) as the forward runs it: batches of pairs in ONE launch (the XCD tile
order of prep_warp_tiled_kernel is taken only when the workgroup count is a multiple of 8), benign and hostile homographies side by side, u8 and float frames,
the block-4 plane output bit for bit against s3_format.h (through tests/frontend_planes.py, which tests/test_frontend_planes_cpu.py holds against the header),
the fast sampler on the steepest 8-bit textures, float frames outside [0, 1], and the float-frame forward against the u8 forward and the oracle."""
import os

import numpy as np
import pytest

import frontend_planes as fpl
from conftest import TOL_COV_REL, tol_px_vs_oracle
from warp_cases import homography_pool, pool_like_kernel

pytestmark = pytest.mark.gpu

IMG_H, IMG_W = 224, 320
F16X2, BF16X3 = 3, 2                       # hnet_config.precision
N_PLANES = {F16X2: 2, BF16X3: 3}
FAST_GATE = 2e-4                           # fast sampler against the bit-faithful one: the project's gate (test_gpu_parity.py), intensity per unit of the frame's range


def pool_like_direct_kernel(x, k):
    """AvgPool in the summation order of prep_kernel (the direct-gather pooling kernel: the exact sampler above K = 2, and frames that are not 16-byte
    aligned): lane j of a window adds its rows 2j, 2j + 1 pixel by pixel, then a pairwise tree over the K / 2 lanes"""
    if k == 1:
        return np.ascontiguousarray(x, dtype=np.float32)
    h, w = x.shape
    lanes = []
    for j in range(k // 2):
        s = np.zeros((h // k, w // k), np.float32)
        for rr in range(2):
            row = x[2 * j + rr::k]
            for a in range(k):
                s = (s + row[:, a::k]).astype(np.float32)
        lanes.append(s)
    while len(lanes) > 1:
        lanes = [(lanes[2 * j] + lanes[2 * j + 1]).astype(np.float32) for j in range(len(lanes) // 2)]
    return (lanes[0] * np.float32(1.0 / (k * k))).astype(np.float32)


def _exact_pool(x, k):
    """the exact sampler's launch for 16-byte aligned frames: the tiled kernel up to K = 2, the direct-gather pooling kernel above"""
    return pool_like_kernel(x, k) if k <= 2 else pool_like_direct_kernel(x, k)


# ---------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def ctxs(blob):
    """contexts by (precision, exact sampler), created on first use; exact = created under HNET_WARP_EXACT=1 as test_gpu_parity.py's eng_exact"""
    from cuahn_vio_amd.homography_net import HnetEngine
    cache = {}

    def get(precision, exact):
        key = (precision, bool(exact))
        if key not in cache:
            old = os.environ.get("HNET_WARP_EXACT")
            if exact:
                os.environ["HNET_WARP_EXACT"] = "1"
            else:
                os.environ.pop("HNET_WARP_EXACT", None)
            try:
                cache[key] = HnetEngine(blob, variant="full", mc_samples=16, dropout_p=0.0, max_batch=8, emit_error_map=True, precision=precision)
            finally:
                if old is None:
                    os.environ.pop("HNET_WARP_EXACT", None)
                else:
                    os.environ["HNET_WARP_EXACT"] = old
            assert bool(cache[key].config().warp_exact) == bool(exact)
        return cache[key]

    yield get
    for e in cache.values():
        e.close()


@pytest.fixture(scope="module")
def frames():
    """16 synthetic pairs as u8 and as the float frames u8 / 255: {"u8": (img1, img2), "f32": (img1, img2)}"""
    from cuahn_vio_amd import synth
    prev, curr, _prior, _ = synth.make_batch(9100, 16)
    f = np.float32(255.0)
    return {"u8": (prev, curr), "f32": ((prev.astype(np.float32) / f), (curr.astype(np.float32) / f))}


@pytest.fixture(scope="module")
def pool():
    return homography_pool()


_DIRECT = {}


def _direct(eng, key, img, hm):
    """warp_f32_kernel (per-pixel global gathers, hnet_op_warp) of one float frame, computed once per (frame, homography) and shared"""
    if key not in _DIRECT:
        d = eng.op_warp(img, hm)
        d.setflags(write=False)
        _DIRECT[key] = d
    return _DIRECT[key]


# ---------------------------------------------------------------------------------------------- a. a batch is its pairs
NAMES16 = ["identity", "z_sign_change", "zoom_out_3x", "z_zero", "far_shift", "shift", "oob", "persp", "dlt4_0", "dlt20_0", "dlt80_0", "rot90", "shrink",
           "edge_minus_half", "dlt20_1", "dlt80_1"]


def _batches_for(n):
    """homography names per batch: every batch of 8 / 16 holds a benign pair, z_sign_change (exact per-pixel path), zoom_out_3x (box beyond WT_CAP: direct
    gathers), z_zero and far_shift; the batches of 1 and of 3 hold them between them"""
    if n == 1:
        return [["identity"], ["z_sign_change"], ["zoom_out_3x"], ["z_zero"], ["far_shift"]]
    if n == 3:
        return [["dlt20_0", "z_sign_change", "zoom_out_3x"], ["z_zero", "far_shift", "persp"]]
    return [NAMES16[:n]]


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [1, 3, 8, 16])
def test_batch_is_its_pairs(ctxs, frames, pool, n, k, exact):
    """n pairs in one launch (35 n workgroups: the XCD tile order for n = 8 and 16, the plain order for 1 and 3) against every pair through the one-pair
    entry, bit for bit; a permutation of the pairs permutes the result; the exact sampler against warp_f32_kernel + AvgPool in the kernel's order; one
    batch per k against the CPU oracle at test_op_prep's gate on the homographies test_op_warp_golden_and_oracle gates"""
    from oracle import pyoracle
    hs_all, gated = pool
    eng = ctxs(F16X2, exact)
    worst_oracle = 0.0
    for bi, names in enumerate(_batches_for(n)):
        idx = [(bi * n + j) % 16 for j in range(n)]
        hs = np.stack([hs_all[nm] for nm in names])
        for fmt in ("u8", "f32"):
            a1, a2 = frames[fmt][0][idx], frames[fmt][1][idx]
            f1, f2 = frames["f32"][0][idx], frames["f32"][1][idx]
            single = eng.op_prep_u8 if fmt == "u8" else eng.op_prep
            for h in (None, hs):
                got = eng.op_prep_batch(a1, a2, h, k)
                assert got.shape == (n, 2, IMG_H // k, IMG_W // k) and np.isfinite(got).all()
                for b in range(n):
                    one = single(a1[b], a2[b], None if h is None else h[b], k)
                    assert np.array_equal(got[b], one), (fmt, names[b] if h is not None else None, b, float(np.abs(got[b] - one).max()))
                if h is None:
                    for b in range(n):
                        want = np.stack([pool_like_kernel(f1[b], k), pool_like_kernel(f2[b], k)])
                        assert np.abs(got[b] - want).max() < 1e-6, (fmt, b)
                    continue
                if n >= 8:
                    perm = np.random.default_rng(100 + n + k).permutation(n)
                    assert not np.array_equal(perm, np.arange(n))
                    moved = eng.op_prep_batch(a1[perm], a2[perm], hs[perm], k)
                    assert np.array_equal(moved, got[perm]), (fmt, float(np.abs(moved - got[perm]).max()))
                if exact:
                    for b in range(n):
                        direct = _direct(eng, ("synth", idx[b], names[b]), f2[b], hs[b])
                        want = np.stack([pool_like_kernel(f1[b], k), pool_like_kernel(direct, k)])
                        if k <= 2:
                            assert np.array_equal(got[b], want), (fmt, names[b], float(np.abs(got[b] - want).max()))
                        else:
                            assert np.abs(got[b] - want).max() < 1e-6, (fmt, names[b])
                if n == 16 and fmt == "u8":
                    for b in range(n):
                        if names[b] in gated:
                            ref = pyoracle.avgpool(np.stack([f1[b], pyoracle.warp(f2[b], hs[b])]), k)
                            d = float(np.abs(got[b] - ref).max())
                            worst_oracle = max(worst_oracle, d)
                            assert d < 2e-4 / k, (names[b], d)
    if n == 16:
        print(f"a: n = 16, k = {k}, {'exact' if exact else 'fast'} sampler: max |prep - oracle| = {worst_oracle:.2e} (gate {2e-4 / k:.1e})")


# ---------------------------------------------------------------------------------------------- b. block-4 planes
B_NAMES = {1: ["dlt20_0"], 3: ["persp", "z_sign_change", "zoom_out_3x"],
           8: ["identity", "z_sign_change", "zoom_out_3x", "z_zero", "far_shift", "persp", "dlt20_0", "edge_minus_half"]}


def _plane_frames(frames, n):
    """u8: the synthetic pairs, pair 0 replaced by a ramp through all 256 values (every frame is k / 255; this one holds every k);
    float: seeded uniform [0, 1) noise blended onto the pairs (not k / 255), the last pair scaled to values below 2^-14 (fp16 subnormal planes)"""
    u1, u2 = frames["u8"][0][:n].copy(), frames["u8"][1][:n].copy()
    ramp = (np.arange(IMG_H * IMG_W) % 256).astype(np.uint8).reshape(IMG_H, IMG_W)
    u1[0], u2[0] = ramp, ramp[::-1]
    rng = np.random.default_rng(4242)
    f1 = (np.float32(0.75) * frames["f32"][0][:n] + np.float32(0.25) * rng.random((n, IMG_H, IMG_W), dtype=np.float32)).astype(np.float32)
    f2 = (np.float32(0.75) * frames["f32"][1][:n] + np.float32(0.25) * rng.random((n, IMG_H, IMG_W), dtype=np.float32)).astype(np.float32)
    f1[n - 1] *= np.float32(2.0 ** -14)
    f2[n - 1] *= np.float32(2.0 ** -14)
    assert f1[n - 1].max() < 2.0 ** -14 and f2[n - 1].max() < 2.0 ** -14 and f1.max() < 1.0
    return {"u8": (u1, u2), "f32": (f1, f2)}


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("precision", [pytest.param(F16X2, id="f16x2"), pytest.param(BF16X3, id="bf16x3")])
def test_block4_planes_are_the_split_of_the_fp32_result(ctxs, frames, pool, precision, exact, n):
    """OUTS3: the planes the launch writes for block 4 - the packed fp16 pair path (prep_f16_residual_pk) in f16x2, split_np in bf16x3, and the route of
    frames that are not 16-byte aligned (prep_k1_kernel + f32_nhwc_to_s3pad_kernel; offset 4: u8 frames 4- but not 16-aligned, offset 1: the byte path) -
    are split2h / split3 of the fp32 result of the same launch without planes, dword for dword; the border keeps the sentinel; the planes join to the fp32
    result (bf16x3: exactly) or to join2h of the expected planes (f16x2)"""
    from cuahn_vio_amd import _capi
    eng = ctxs(precision, exact)
    n_planes = N_PLANES[precision]
    hs = np.stack([pool[0][nm] for nm in B_NAMES[n]])
    pf = _plane_frames(frames, n)
    py, px = _capi.B4_PADY, _capi.B4_PADX
    border = np.ones((_capi.B4_HP, _capi.B4_WP), bool)
    border[py:py + IMG_H, px:px + IMG_W] = False
    for fmt, offsets in (("u8", (0, 4, 1)), ("f32", (0, 4))):
        a1, a2 = pf[fmt]
        for off in offsets:
            plain = eng.op_prep_batch(a1, a2, hs, 1, align_off=off)
            joined, planes = eng.op_prep_batch(a1, a2, hs, 1, align_off=off, want_planes=True)
            assert planes.shape == (n_planes, n, _capi.B4_HP, _capi.B4_WP) and np.isfinite(plain).all()
            want, want_joined = fpl.expected_planes(plain, n_planes)
            inner = planes[:, :, py:py + IMG_H, px:px + IMG_W]
            bad = inner != want
            assert not bad.any(), (fmt, off, int(bad.sum()), [tuple(int(v) for v in p) for p in np.argwhere(bad)[:4]],
                                   [hex(int(v)) for v in inner[bad][:4]], [hex(int(v)) for v in want[bad][:4]])
            assert (planes[:, :, border] == _capi.B4_SENTINEL).all(), (fmt, off, "the launch wrote into the border of the plane layout")
            if n_planes == 3:
                assert np.array_equal(joined, plain), (fmt, off)
            assert np.array_equal(joined, want_joined), (fmt, off)
    assert eng.precision() == precision


def test_prep_batch_rejects_what_it_cannot_run(ctxs, frames, blob):
    from cuahn_vio_amd.homography_net import HnetEngine, HnetError
    eng = ctxs(F16X2, False)
    a1, a2 = frames["u8"][0][:1], frames["u8"][1][:1]
    h = np.eye(3, dtype=np.float32)[None]
    for kwargs in (dict(h=h, k=2, want_planes=True), dict(h=None, k=1, want_planes=True), dict(h=h, k=3), dict(h=h, k=1, align_off=16)):
        with pytest.raises(HnetError) as ei:
            eng.op_prep_batch(a1, a2, **kwargs)
        assert ei.value.status == 1                                   # HNET_ERR_INVALID_ARG
    with pytest.raises(HnetError) as ei:
        eng.op_prep_batch(frames["f32"][0][:1], frames["f32"][1][:1], h, 1, align_off=1)      # a float frame at an odd address
    assert ei.value.status == 1
    fp32 = HnetEngine(blob, variant="full", mc_samples=16, dropout_p=0.0, max_batch=1, precision=0)   # exact-fp32 MFMA mode: no block-4 plane input
    try:
        with pytest.raises(HnetError) as ei:
            fp32.op_prep_batch(a1, a2, h, 1, want_planes=True)
        assert ei.value.status == 6                                   # HNET_ERR_UNSUPPORTED
        assert np.array_equal(fp32.op_prep_batch(a1, a2, h, 1), eng.op_prep_batch(a1, a2, h, 1))
    finally:
        fp32.close()


# ---------------------------------------------------------------------------------------------- c. steepest textures
def _textures():
    yy, xx = np.mgrid[0:IMG_H, 0:IMG_W]
    dots = np.zeros((IMG_H, IMG_W), np.uint8)
    for y, x in ((0, 0), (0, IMG_W - 1), (IMG_H - 1, 0), (IMG_H - 1, IMG_W - 1), (0, IMG_W // 2), (IMG_H - 1, IMG_W // 2), (IMG_H // 2, 0),
                 (IMG_H // 2, IMG_W - 1)):
        dots[y, x] = 255
    return {"checker": (((xx + yy) & 1) * 255).astype(np.uint8), "stripes_x": ((xx & 1) * 255).astype(np.uint8),
            "stripes_y": ((yy & 1) * 255).astype(np.uint8), "all255": np.full((IMG_H, IMG_W), 255, np.uint8), "dots": dots}


TEXTURES = _textures()


def _fast_against_exact(ctxs, pool, tag, img_u8, img_f32, k, gate, ch0_between_samplers, interior=None):
    """one frame under every homography of the pool (two launches of ten pairs per sampler and pixel format).  The exact context against warp_f32_kernel +
    AvgPool in its kernel's order: bitwise.  The default context: channel 0 (img1, not warped) bitwise AvgPool in the tiled kernel's order - and, where the
    sums are exact in any order (ch0_between_samplers: frames of 0 and 1), bitwise the exact context's; channel 1 within `gate` of the exact context's.
    interior: None, or a function (name, H) -> mask of the output pixels to measure apart (K = 1).
    Returns (worst difference, its homography, failures, worst difference inside the masks): the caller asserts after everything was measured"""
    hs_all, _gated = pool
    names = list(hs_all)
    fast, ex = ctxs(F16X2, False), ctxs(F16X2, True)
    worst, worst_name, failures, worst_in = 0.0, None, [], 0.0
    ch0_fast, ch0_exact = pool_like_kernel(img_f32, k), _exact_pool(img_f32, k)
    for fmt, img in (("u8", img_u8), ("f32", img_f32)):
        if img is None:
            continue
        for lo in range(0, len(names), 10):
            part = names[lo:lo + 10]
            hs = np.stack([hs_all[nm] for nm in part])
            a = np.repeat(img[None], len(part), axis=0)
            got_f, got_e = fast.op_prep_batch(a, a, hs, k), ex.op_prep_batch(a, a, hs, k)
            for b, nm in enumerate(part):
                direct = _direct(ex, (tag, nm), img_f32, hs[b])
                want = np.stack([ch0_exact, _exact_pool(direct, k)])
                if not np.array_equal(got_e[b], want):
                    failures.append((fmt, nm, "exact sampler != warp_f32_kernel", float(np.abs(got_e[b] - want).max())))
                if not (np.isfinite(got_f[b]).all() and np.array_equal(got_f[b, 0], ch0_fast)):
                    failures.append((fmt, nm, "channel 0 of the default context is not the pooled img1"))
                if ch0_between_samplers and not np.array_equal(got_f[b, 0], got_e[b, 0]):
                    failures.append((fmt, nm, "channel 0 differs between the samplers"))
                d = float(np.abs(got_f[b, 1] - got_e[b, 1]).max())
                if d > worst:
                    worst, worst_name = d, nm
                if not d < gate:
                    failures.append((fmt, nm, "fast sampler beyond its gate", d))
                if interior is not None:
                    m = interior(nm, hs[b])
                    if m.any():
                        worst_in = max(worst_in, float(np.abs(got_f[b, 1] - got_e[b, 1])[m].max()))
    return worst, worst_name, failures, worst_in


@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("texture", list(TEXTURES))
def test_fast_sampler_on_the_steepest_textures(ctxs, pool, texture, k):
    """1-px checkerboard and stripes of 0 / 255 (a gradient of 1 per pixel and axis, the steepest an 8-bit frame has), a saturated frame (the zero padding
    is its only edge) and single bright pixels on the image's corners and edges, under every homography of the pool.
    Measured on an MI355X (K = 1, the worst K): checkerboard 1.20e-4, stripes 1.22e-4 / 9.6e-5, saturated 1.22e-4, dots 4.4e-5; the stripes away from the
    zero padding give the samplers' position difference itself: 1.22e-4 px in x, 6.1e-5 px in y"""
    img = TEXTURES[texture]
    f32 = (img.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    interior = None
    if k == 1 and texture.startswith("stripes"):
        # where all four taps lie inside the image (a saturated frame warps to 1 there) the bilinear blend of 1-px stripes of 0 / 1 is the fractional
        # sampling position across the stripes, or 1 minus it: the intensity difference between the samplers is their position difference in that axis
        ones = np.ones((IMG_H, IMG_W), np.float32)
        ex = ctxs(F16X2, True)

        def interior(nm, hm):
            return np.abs(_direct(ex, ("ones", nm), ones, hm) - np.float32(1.0)) < 1e-6
    worst, name, failures, worst_in = _fast_against_exact(ctxs, pool, texture, img, f32, k, FAST_GATE, True, interior)
    print(f"c: texture {texture}, k = {k}: fast vs exact sampler, max intensity difference {worst:.3e} (at {name}; gate {FAST_GATE:.0e})")
    if interior is not None:
        print(f"c: texture {texture}: sampling position difference across the stripes, away from the zero padding: {worst_in:.3e} px")
    assert not failures, failures[:8]


# ---------------------------------------------------------------------------------------------- d. float frames outside [0, 1]
@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("kind", ["minus3_to_5", "magnitude_1e4"])
def test_float_frames_outside_the_unit_range(ctxs, frames, pool, kind, k):
    """nothing in the float instantiations may assume [0, 1]: the exact sampler stays bitwise warp_f32_kernel, the fast one within 2e-4 of the frame's range"""
    unit = frames["f32"][1][3]
    img = (unit * np.float32(8.0) - np.float32(3.0)).astype(np.float32) if kind == "minus3_to_5" else ((unit - np.float32(0.5)) * np.float32(2.0e4)).astype(np.float32)
    span = float(img.max() - img.min())
    worst, name, failures, _ = _fast_against_exact(ctxs, pool, kind, None, img, k, FAST_GATE * span, False)
    print(f"d: float frame {kind} (range {span:.4g}), k = {k}: fast vs exact sampler, max difference {worst:.3e} = {worst / span:.3e} of the range "
          f"(at {name}; gate {FAST_GATE:.0e} of the range)")
    assert not failures, failures[:8]


# ---------------------------------------------------------------------------------------------- e. float-frame forward
@pytest.fixture(scope="module")
def frames40(frames):
    """40 distinct pairs from the 16 synthetic ones (the second and third sets are the first flipped), with priors"""
    from cuahn_vio_amd import synth
    p, c = frames["u8"]
    prev = np.ascontiguousarray(np.concatenate([p, p[:, ::-1], p[:8, :, ::-1]]))
    curr = np.ascontiguousarray(np.concatenate([c, c[:, ::-1], c[:8, :, ::-1]]))
    prior = np.stack([synth.make_prior(9100 + i, synth.true_offsets(9100 + i % 16)) * np.float32(1.0 if i < 16 else 0.25) for i in range(40)]).astype(np.float32)
    return prev, curr, prior


@pytest.mark.parametrize("precision", [pytest.param(F16X2, id="f16x2"), pytest.param(BF16X3, id="bf16x3")])
@pytest.mark.parametrize("variant", ["full", "prior3"])
def test_float_frames_give_the_u8_forward_bitwise(blob, frames40, variant, precision):
    """float frames equal to u8 / 255 through the whole forward - prep (batches 1 and 5: the latency path with prep_fc<float>; 9 and 40: separate launches),
    errmap_kernel<float> - give mean, cov and error map of the u8 frames bit for bit, from host buffers and from device buffers"""
    import torch
    from cuahn_vio_amd.homography_net import PIX_F32, PIX_U8, HnetEngine
    prev, curr, prior = frames40
    eng = HnetEngine(blob, variant=variant, mc_samples=16, dropout_p=0.05, mc_seed=7, max_batch=40, emit_error_map=True, precision=precision)
    dev = torch.device("cuda:0")
    try:
        for B in (1, 5, 9, 40):
            pu, cu = prev[:B], curr[:B]
            pf, cf = pu.astype(np.float32) / np.float32(255.0), cu.astype(np.float32) / np.float32(255.0)
            pr = prior[:B] if variant == "prior3" else None
            want = eng.infer_batch(pu, cu, pr, pair_seq0=11, want_err=True)
            got = eng.infer_batch(pf, cf, pr, pair_seq0=11, want_err=True)
            assert np.isfinite(want[0]).all() and np.abs(want[0]).max() > 0.1 and want[2].max() > 1.0
            for name, w, g in zip(("mean", "cov", "error map"), want, got):
                assert np.array_equal(w, g), (B, "host", name, float(np.abs(w - g).max()))
            res = {}
            for fmt, a, b in ((PIX_U8, pu, cu), (PIX_F32, pf, cf)):
                tp, tc = torch.from_numpy(np.ascontiguousarray(a)).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev)
                tpr = torch.from_numpy(pr).to(dev) if pr is not None else None
                mean, cov, err = torch.zeros(B, 8, device=dev), torch.zeros(B, 64, device=dev), torch.zeros(B, IMG_H, IMG_W, device=dev)
                torch.cuda.synchronize()
                eng.infer_batch_device(tp.data_ptr(), tc.data_ptr(), fmt, tpr.data_ptr() if tpr is not None else None, B, 11, mean.data_ptr(), cov.data_ptr(),
                                       err.data_ptr())
                eng.synchronize()
                res[fmt] = (mean.cpu().numpy(), cov.cpu().numpy(), err.cpu().numpy())
            assert np.isfinite(res[PIX_U8][0]).all() and np.abs(res[PIX_U8][0]).max() > 0.1 and res[PIX_U8][2].max() > 1.0
            for name, w, g in zip(("mean", "cov", "error map"), res[PIX_U8], res[PIX_F32]):
                assert np.array_equal(w, g), (B, "device", name, float(np.abs(w - g).max()))
        assert eng.precision() == precision
    finally:
        eng.close()


_ORACLE_FWD = {}


@pytest.mark.parametrize("precision", [pytest.param(F16X2, id="f16x2"), pytest.param(BF16X3, id="bf16x3")])
def test_float_frames_forward_against_the_oracle(blob, oracle, frames, precision):
    """float frames that are no k / 255 (seeded uniform noise blended onto synthetic pairs), prior-3 model, batch 3: every pair against the oracle on the same
    float frames - offsets, covariance, error map"""
    from cuahn_vio_amd import synth
    from cuahn_vio_amd.homography_net import HnetEngine
    rng = np.random.default_rng(777)
    pf = (np.float32(0.75) * frames["f32"][0][:3] + np.float32(0.25) * rng.random((3, IMG_H, IMG_W), dtype=np.float32)).astype(np.float32)
    cf = (np.float32(0.75) * frames["f32"][1][:3] + np.float32(0.25) * rng.random((3, IMG_H, IMG_W), dtype=np.float32)).astype(np.float32)
    assert pf.max() < 1.0 and pf.min() >= 0.0 and not np.array_equal(np.round(pf * 255) / 255, pf)
    prior = np.stack([synth.make_prior(9100 + i, synth.true_offsets(9100 + i)) for i in range(3)]).astype(np.float32)
    eng = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=7, max_batch=3, emit_error_map=True, precision=precision)
    try:
        mean, cov, err = eng.infer_batch(pf, cf, prior, pair_seq0=5, want_err=True)
        assert eng.precision() == precision
    finally:
        eng.close()
    for b in range(3):
        if b not in _ORACLE_FWD:
            _ORACLE_FWD[b] = oracle.forward(pf[b], cf[b], prior[b], 3, 16, 0.05, 7, 5 + b, want_err=True)
        o = _ORACLE_FWD[b]
        d = float(np.abs(mean[b] - o["mean"]).max())
        dc = float(np.abs(cov[b] - o["cov"]).max() / np.abs(o["cov"]).max())
        de = float(np.abs(err[b][::4, ::4] - o["err"][::4, ::4]).max())
        ds = float(abs(err[b].astype(np.float64).sum() - o["err"].astype(np.float64).sum()) / o["err"].astype(np.float64).sum())
        print(f"e: float pair {b}: |hip - oracle| = {d:.2e} px, cov rel {dc:.2e}, error map max {de:.2e}, sum rel {ds:.2e}")
        assert d < tol_px_vs_oracle(precision) and dc < TOL_COV_REL, (b, d, dc)
        assert de < 0.1 and ds < 2e-5, (b, de, ds)
