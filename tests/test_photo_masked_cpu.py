"""The robust photometric alignment on the template pixels a mask admits (include/hnet.h hnet_op_photo_align_masked; include/hnet_photo_masked.h; DESIGN
7ae) on the CPU: the mask pyramid and its counts against numpy, the host reference tests/cpp/photo_masked_ref.cpp against the robust reference (a full
mask: byte for byte), img1 under refused bytes, the empty mask, the composite rows (a camera between stored keyframes against their rendered composite:
with the mask, and with the existing alignment on the same composite), and the reference under AddressSanitizer + UBSan
(tests/cpp/photo_masked_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import keyframe_localise_util as KL
import keyframe_render_util as KR
import photo_align_pyr_util as P
import photo_align_util as U
import photo_masked_util as M
import photo_robust_util as R

ROOT = U.ROOT


@pytest.fixture(scope="module")
def mref(tmp_path_factory):
    return M.build_ref(tmp_path_factory.mktemp("photo_masked_ref"))


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return R.build_ref(tmp_path_factory.mktemp("photo_masked_robust_ref"))


@pytest.fixture(scope="module")
def render_ref(tmp_path_factory):
    return KR.build_ref(tmp_path_factory.mktemp("photo_masked_render_ref"))


@pytest.fixture(scope="module")
def pair():
    i1, i2, _ = U.smooth_pair(1, 2.0)
    return i1, i2


def test_mask_pyramid_and_counts_match_numpy(mref, render_ref):
    """levels 1 - 3 (bytes 0 / 1, the AND of the 4^L level-0 bytes under a pixel, packed like the image pyramid) and n_mask [4][7] of every mask of the GPU
    test, the cover of the two-keyframe composite among them, equal the numpy restatement; every byte is written"""
    cases = dict(M.masks())
    cases["two-keyframe-cover"] = KL.composite(render_ref, "two-keyframes-drift8", 1)[1]
    pyr, n_mask = M.ref_pyramid(mref, np.stack(list(cases.values())))
    for i, (name, mask) in enumerate(cases.items()):
        lv, n = M.numpy_mask_pyramid(mask)
        got = P.split_pyramid(pyr[i])
        for L in (1, 2, 3):
            assert got[L - 1].tobytes() == lv[L].tobytes(), (name, L)
        assert n_mask[i].tobytes() == n.tobytes(), (name, n_mask[i], n)
    assert not M.numpy_mask_pyramid(cases["checkerboard"])[1][1:].any() and M.numpy_mask_pyramid(cases["rows-0-95-zero"])[1][:, :3].sum() == 0
    assert 0.6 < (cases["two-keyframe-cover"] != 0).mean() < 0.9


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_full_mask_is_the_robust_reference(mref, rref, levels):
    """a mask of all 255 gives photo_robust_ref_run's records byte for byte, out and every level, on a clean and on a spoiled pair"""
    b1, b2, _, bs = R.row_pairs("block-4levels")
    s1, s2, _ = U.smooth_pair(5, 8.0)
    i1, i2, start = np.stack([b1[0], s1]), np.stack([b2[0], s2]), np.stack([bs[0], np.zeros(8, np.float32)])
    want, wlv = R.ref_run(rref, i1, i2, start, levels, max_iterations=8)
    out, lv = M.ref_run(mref, i1, np.full_like(i1, 255), i2, start, levels, max_iterations=8)
    assert out.tobytes() == want.tobytes() and lv.tobytes() == wlv.tobytes()
    assert (lv["px"]["trials"] > 0).any()


def test_img1_under_refused_bytes_is_never_read(mref, pair):
    """bytes of img1 under zero mask bytes do not change a bit of any level's record, for every mask, under both option sets"""
    i1, i2 = pair
    for name, mask in M.masks().items():
        for kw in (dict(), dict(min_valid=M.SPARSE_MIN_VALID)):
            a = M.ref_run(mref, i1, mask, i2, np.zeros(8, np.float32), 4, **kw)
            b = M.ref_run(mref, M.scramble_under(i1, mask), mask, i2, np.zeros(8, np.float32), 4, **kw)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (name, kw)


def test_masks_stop_or_run_as_their_counts_say(mref, pair):
    """an all-zero mask stops FEW_PIXELS at every level with n_valid = 0 and a zero record, also with min_valid = 0; a checkerboard has empty levels 1 - 3
    (FEW_PIXELS) and runs level 0 from the call's start; one zero byte costs exactly the pixels it touches; n_valid never exceeds the mask's count"""
    i1, i2 = pair
    zero = np.zeros(8, np.float32)
    for mv in (0, 20000):
        _, lv = M.ref_run(mref, i1, M.masks()["all-zero"], i2, zero, 4, min_valid=mv)
        assert (lv["px"]["flags"] == U.FEW_PIXELS).all() and not lv["px"]["n_valid0"].any() and not lv["px"]["n_valid"].any() and not lv["n_outliers0"].any()
        assert not lv["info10"].any() and not lv["grad10"].any() and not lv["px"]["mse0"].any() and (lv["px"]["trials"] == 0).all()
    _, lv = M.ref_run(mref, i1, M.masks()["checkerboard"], i2, zero, 4)
    assert (lv[0, 1:]["px"]["flags"] == U.FEW_PIXELS).all() and not lv[0, 1:]["px"]["n_valid0"].any()
    assert lv[0, 0]["px"]["trials"] > 0 and lv[0, 0]["px"]["n_valid0"] > 20000 and not (lv[0, 0]["px"]["flags"] & U.FEW_PIXELS)
    _, full = M.ref_run(mref, i1, M.masks()["full"], i2, zero, 4, max_iterations=0)
    _, one = M.ref_run(mref, i1, M.masks()["one-zero-byte"], i2, zero, 4, max_iterations=0)
    assert [int(f) - int(o) for f, o in zip(full[0]["px"]["n_valid0"], one[0]["px"]["n_valid0"])] == [1, 1, 1, 1]      # (one pixel of every level holds the byte)
    for name, mask in M.masks().items():
        _, n = M.numpy_mask_pyramid(mask)
        _, lv = M.ref_run(mref, i1, mask, i2, zero, 4, min_valid=0)
        for L in range(4):
            assert lv[0, L]["px"]["n_valid0"] <= n[L].sum() and lv[0, L]["px"]["n_valid"] <= n[L].sum(), (name, L)


def _composite_row(mref, rref, render_ref, name):
    """-> per seed (before, after masked, after unmasked, masked record, unmasked record, cover fraction), all distances worst corner component in px"""
    rows = []
    for seed in KL.SEEDS:
        s = KL.scene(name, seed)
        comp, cover, rec = KL.composite(render_ref, name, seed)
        zero = np.zeros(8, np.float32)
        masked = M.ref_run(mref, comp, cover, s["frame"], zero, KL.LEVELS, max_iterations=KL.TRIALS)[0][0]
        plain = R.ref_run(rref, comp, s["frame"], zero, KL.LEVELS, max_iterations=KL.TRIALS)[0][0]
        rows.append((KL.worst_corner_px(zero, s["truth"]), KL.worst_corner_px(masked["px"]["offsets_px"], s["truth"]),
                     KL.worst_corner_px(plain["px"]["offsets_px"], s["truth"]), masked, plain, float(rec["n_covered"][0]) / U.NPIX))
    return rows


@pytest.mark.parametrize("name", list(KL.ROWS))
def test_composite_rows(mref, rref, render_ref, name):
    """a camera between stored keyframes against the FEWEST_LINKS composite of the keyframes in the view its chain predicts, the cover image as the mask,
    from zero offsets, 3 levels, 6 trials, robust defaults, seeds 1, 2, 5, 11: the masked alignment ends within the row's gate (TWICE the worst value this
    test prints) of the truth and every drift-8 start lies at least three gates off; on the two-keyframe rows (cover about 0.75) the masked mean cost is
    below 10 and the existing alignment's on the same composite above 100, and the masked result is nearer the truth for every seed; with four keyframes
    that cover the view there is nothing to mask and the two agree byte for byte.  Every entry's grid count in the predicted view is below 32, so the
    existing revisit's select (keyframe_map_util.np_select, min_grid = 32, every entry eligible) has no candidate: these are scenes it cannot serve"""
    rows = _composite_row(mref, rref, render_ref, name)
    gate = KL.GATES[name]
    for seed in KL.SEEDS:
        slot, grids = KL.revisit_select(name, seed)
        print(f"{name} seed {seed}: grid counts of the entries {grids}, np_select with min_grid {KL.MIN_GRID} -> slot {slot}")
        assert slot == -1 and all(0 <= g < KL.MIN_GRID for g in grids), (name, seed, grids)
    for seed, (before, after, after_plain, masked, plain, cover) in zip(KL.SEEDS, rows):
        print(f"{name} seed {seed}: cover {cover:.3f}, before {before:.3f} px, masked {after:.4f} px (mse {masked['px']['mse']:.2f}, n_valid "
              f"{masked['px']['n_valid']}, flags {masked['px']['flags']}), existing alignment {after_plain:.4f} px (mse {plain['px']['mse']:.1f}, outliers "
              f"{plain['n_outliers']})")
    print(f"{name}: worst masked {max(r[1] for r in rows):.4f} px, gate {gate:.4f} px")
    for seed, (before, after, after_plain, masked, plain, cover) in zip(KL.SEEDS, rows):
        assert after < gate, (name, seed, after)
        assert not (masked["px"]["flags"] & (U.SINGULAR | U.DEGENERATE | U.FEW_PIXELS)), (name, seed)
        if KL.ROWS[name][1] > 0.0:
            assert before >= KL.BEFORE_GATES * gate, (name, seed, before)
        if name.startswith("two-keyframes"):
            assert 0.6 < cover < 0.9
            assert masked["px"]["mse"] < KL.MASKED_MSE_BELOW and plain["px"]["mse"] > KL.UNMASKED_MSE_ABOVE, (name, seed)
            assert after < after_plain, (name, seed, after, after_plain)
        else:
            assert cover == 1.0 and masked.tobytes() == plain.tobytes(), (name, seed)
    assert gate <= 2 * max(r[1] for r in rows) * 1.01, "KL.GATES holds no more than twice the worst value printed above"


def test_photo_masked_check_under_asan_ubsan(tmp_path):
    """the reference and the header on hostile masks and starts under AddressSanitizer + UBSan: a stand-alone program; nothing loaded into python is
    sanitized"""
    exe = str(tmp_path / "photo_masked_check_san.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *U.HOST_FLAGS,
                    os.path.join(ROOT, "tests", "cpp", "photo_masked_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "photo_masked_check: ok" in r.stdout
