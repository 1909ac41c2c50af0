"""Photometric residual records (include/hnet.h hnet_photo_residual) on the CPU: the host reference tests/cpp/photo_ref.cpp - the sampler of
csrc/warp_dev.h restated in host fp32 on csrc/geom.h's dlt_solve - pinned to the reference model's recorded error sums, its closed-form cases, and its core
under AddressSanitizer + UBSan (tests/cpp/photo_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import golden_cases, load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPIX = 224 * 320
DEGENERATE = 1
HOST_FLAGS = ["-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "cuahn_vio_amd", "csrc")]
REC = np.dtype([("sum", "<f8"), ("sum_inside", "<f8"), ("n_inside", "<i4"), ("flags", "<i4")])


def build_photo_ref(tmp):
    so = str(tmp / "photo_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", *HOST_FLAGS, os.path.join(ROOT, "tests", "cpp", "photo_ref.cpp"), "-o", so],
                   check=True)
    return C.CDLL(so)


def photo_ref_records(lib, img1, img2, offsets, want_map=False):
    """-> records [n, m], n_edge [n, m](, map [n, m, 224, 320])"""
    a = np.ascontiguousarray(img1, np.uint8).reshape(-1, 224, 320)
    b = np.ascontiguousarray(img2, np.uint8).reshape(-1, 224, 320)
    n = a.shape[0]
    off = np.ascontiguousarray(offsets, np.float32).reshape(n, -1, 8)
    m = off.shape[1]
    out, edge = np.zeros((n, m), REC), np.zeros((n, m), np.int32)
    emap = np.zeros((n, m, 224, 320), np.float32) if want_map else None
    lib.photo_ref_records(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), n, C.c_void_p(off.ctypes.data), m, C.c_void_p(out.ctypes.data),
                          C.c_void_p(edge.ctypes.data), C.c_void_p(emap.ctypes.data) if want_map else None)
    return (out, edge, emap) if want_map else (out, edge)


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return build_photo_ref(tmp_path_factory.mktemp("photo_ref"))


def _pin_cases():
    out = []
    for name in golden_cases():
        g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        if "err_stats64" in g.files and str(g["kind"]) in ("pair", "replay", "noise"):
            out.append(name)
    return out


@pytest.mark.parametrize("name", _pin_cases())
def test_reference_pin(pref, name):
    """1. the record of the golden's mean64 on the case's frames carries the reference model's own error sum (err_stats64[0]); the gate of
    test_gpu_parity.py's error map.  Measured over all cases: 1.3e-6 at worst (mean64 rounded to the fp32 offsets the C ABI takes)"""
    g, i1, i2, _prior, _btr = load_case(name)
    assert i1.dtype == np.uint8 and i2.dtype == np.uint8
    rec, _ = photo_ref_records(pref, i1, i2, g["mean64"])
    rel = abs(rec["sum"][0, 0] - g["err_stats64"][0]) / g["err_stats64"][0]
    print(f"{name}: sum {rec['sum'][0, 0]:.6f} vs err_stats64 {g['err_stats64'][0]:.6f}: {rel:.2e}")
    assert rec["flags"][0, 0] == 0
    assert rel < 2e-5


def test_pin_covers_every_golden_with_err_stats64():
    """(the pin leaves out only goldens whose frames are not 8-bit images: the constant float pairs)"""
    have = [n for n in golden_cases() if "err_stats64" in np.load(os.path.join(ROOT, "tests", "golden", n + ".npz")).files]
    left = sorted(set(have) - set(_pin_cases()))
    assert all(n.startswith("const_") for n in left), left
    assert len(_pin_cases()) >= 20


def _round_trip(n):
    """grid_sample's sampling position of pixel index 0 .. n - 1 under the identity, in the number formats the sampler is specified in (csrc/warp_dev.h
    warp_coords): g = fma(u, fl32(2 / (n - 1)), -1), then ((g + 1) * 0.5) * (n - 1), every operation rounded to fp32.  The fma is formed in float64, where
    the product (9 x 24 bits) and the sum are exact, and rounded once."""
    u = np.arange(n, dtype=np.float64)
    c = np.float64(np.float32(2.0 / (n - 1)))
    g = (u * c - 1.0).astype(np.float32)
    return ((g + np.float32(1.0)) * np.float32(0.5)) * np.float32(n - 1)


def _bilinear64(img, ix, iy):
    """zeros-padded bilinear sample of a u8 image / 255 at the positions (ix [320], iy [224]) in float64"""
    p = np.zeros((226, 322))
    p[1:-1, 1:-1] = img.astype(np.float64) / 255.0
    x0, y0 = np.floor(ix).astype(int), np.floor(iy).astype(int)
    wx, wy = (ix - np.floor(ix)).astype(np.float64)[None, :], (iy - np.floor(iy)).astype(np.float64)[:, None]
    X, Y = x0[None, :] + 1, y0[:, None] + 1
    return (p[Y, X] * (1 - wx) + p[Y, X + 1] * wx) * (1 - wy) + (p[Y + 1, X] * (1 - wx) + p[Y + 1, X + 1] * wx) * wy


def test_identity(pref):
    """2. zero offsets: every pixel inside, sum == sum_inside, flags 0.
    The sum equals the integer sum |img2 - img1| of the u8 frames EXACTLY where every sample is exact: with img2 = 0 every tap is 0 and
    e = fl(fl(a / 255) * 255) = a for every byte a (asserted below for all 256).  On a textured img2 the equality cannot be exact with the sampler the
    records must share with the error map: grid_sample's fp32 normalise / un-normalise round trip leaves the sampling position up to a few ulp of 319
    off the pixel centre, so each sample blends in ~1e-5 of a neighbour (measured on synth seed 1: sum 1 778 749.682 vs 1 778 750, -1.8e-7 relative).
    That case is pinned to what the round trip predicts: the positions follow from the number formats alone (_round_trip), a float64 bilinear sample at
    them gives the sum the sampler must produce, and what is left is the fp32 rounding of one e: two table values, the weight product, four FMAs, the
    difference and the scaling, at most 8 roundings of 2^-24 on values <= 1, times 255, per pixel - 8.7 over the image in the worst case."""
    from cuahn_vio_amd import synth
    i1, i2, _ = synth.make_pair(1)
    zero = np.zeros(8, np.float32)
    ramp = np.arange(NPIX, dtype=np.int64).reshape(224, 320)
    every_byte = ((ramp * 7 + ramp // 320) % 256).astype(np.uint8)            # all 256 values, many times over
    assert len(np.unique(every_byte)) == 256
    for a in (i1, every_byte):
        rec, edge = photo_ref_records(pref, a, np.zeros_like(a), zero)
        r = rec[0, 0]
        assert r["n_inside"] == NPIX and r["flags"] == 0 and edge[0, 0] == 0
        assert r["sum"] == r["sum_inside"] == float(a.astype(np.int64).sum())
    rec, edge = photo_ref_records(pref, i1, i2, zero)
    r = rec[0, 0]
    want = float(np.abs(i2.astype(np.int64) - i1.astype(np.int64)).sum())
    ix, iy = _round_trip(320), _round_trip(224)
    assert np.abs(ix - np.arange(320)).max() <= 4 * 2.0 ** -15 and np.abs(iy - np.arange(224)).max() <= 4 * 2.0 ** -16      # "a few ulp", far from 0.5
    predicted = float((np.abs(_bilinear64(i2, ix, iy) - i1.astype(np.float64) / 255.0) * 255.0).sum())
    bound = NPIX * 8 * 2.0 ** -24 * 255
    print(f"identity on synth seed 1: sum {r['sum']:.6f}; integer sum {want:.0f} ({r['sum'] - want:+.4f}); predicted from the round trip {predicted:.6f} "
          f"({r['sum'] - predicted:+.6f}, bound {bound:.2f})")
    assert r["n_inside"] == NPIX and r["flags"] == 0 and edge[0, 0] == 0
    assert r["sum"] == r["sum_inside"]
    assert abs(r["sum"] - predicted) <= bound


def test_out_of_bounds_shift(pref):
    """3. +100.25 px in u: columns 0 - 219 sample ix <= 319.25 < 319.5; in the other columns every tap is outside, so e = img1 * 255 up to the LUT rounding"""
    from cuahn_vio_amd import synth
    i1, i2, _ = synth.make_pair(1)
    off = np.tile(np.array([100.25, 0.0], np.float32), 4)
    rec, edge, emap = photo_ref_records(pref, i1, i2, off, want_map=True)
    r = rec[0, 0]
    assert r["n_inside"] == 224 * 220 and r["flags"] == 0 and edge[0, 0] == 0
    outside = float(i1[:, 220:].astype(np.int64).sum())
    assert abs((r["sum"] - r["sum_inside"]) - outside) <= 1e-6 * outside
    assert r["sum"] == pytest.approx(float(emap[0, 0].astype(np.float64).sum()), rel=1e-10)


def test_degenerate_and_nan(pref):
    """4. a quadrilateral with all corners on one line (det = 0) and NaN offsets: the flag, finite sums, nothing inside"""
    from cuahn_vio_amd import synth
    i1, i2, _ = synth.make_pair(1)
    p4 = np.array([0, 0, 0, 223, 319, 223, 319, 0], np.float32)
    line = np.array([0, 0, 10, 5, 20, 10, 30, 15], np.float32) - p4
    nan = np.zeros(8, np.float32)
    nan[3] = np.nan
    rec, edge = photo_ref_records(pref, i1, i2, np.stack([line, nan, np.zeros(8, np.float32)]))
    for c in (0, 1):
        r = rec[0, c]
        assert r["flags"] == DEGENERATE and r["n_inside"] == 0 and r["sum_inside"] == 0.0 and np.isfinite(r["sum"])
        assert r["sum"] == float(i1.astype(np.int64).sum())                  # every sample is 0: e = img1 * 255
    assert rec[0, 2]["flags"] == 0 and rec[0, 2]["n_inside"] == NPIX


def test_photo_check_under_asan_ubsan(tmp_path):
    """5. the reference's core on fixed inputs under AddressSanitizer + UBSan (a stand-alone program)"""
    exe = str(tmp_path / "photo_check_san.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *HOST_FLAGS,
                    os.path.join(ROOT, "tests", "cpp", "photo_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "photo_check: ok" in r.stdout


def test_truth_beats_identity(pref):
    """6. synth.make_pair(1) moves its corners by up to 11.4 px: the record of the pair's true offsets has a mean inside residual far below the identity's.
    Measured with photo_ref: ratio 0.193 (seeds 1 - 19 at max_offset 12: 0.17 - 0.30)"""
    from cuahn_vio_amd import synth
    i1, i2, off = synth.make_pair(1)
    rec, _ = photo_ref_records(pref, i1, i2, np.stack([np.zeros(8), off]))
    res = rec["sum_inside"][0] / rec["n_inside"][0]
    print(f"mean inside residual: identity {res[0]:.3f}, truth {res[1]:.3f}, ratio {res[1] / res[0]:.3f}")
    assert res[1] / res[0] < 0.8


def test_program_prints_records(tmp_path, pref):
    """the stand-alone program reads frames and offsets and prints the library's records and n_edge"""
    from cuahn_vio_amd import synth
    i1, i2, off = synth.make_pair(2)
    offs = np.stack([np.zeros(8), off, np.tile([-0.5, 0.0], 4)]).astype(np.float32)      # (the last one puts column 0 on the inside bound)
    exe, inp = str(tmp_path / "photo_ref.bin"), str(tmp_path / "in.bin")
    subprocess.run(["g++", "-std=c++17", "-O2", "-DPHOTO_REF_MAIN", *HOST_FLAGS, os.path.join(ROOT, "tests", "cpp", "photo_ref.cpp"), "-o", exe], check=True)
    with open(inp, "wb") as f:
        f.write(np.array([1, 3], np.int32).tobytes() + i1.tobytes() + i2.tobytes() + offs.tobytes())
    out = subprocess.run([exe, inp], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    rec, edge = photo_ref_records(pref, i1, i2, offs)
    for c in range(3):
        w = out[c].split()
        assert [int(w[0]), int(w[1])] == [0, c]
        assert float(w[2]) == rec["sum"][0, c] and float(w[3]) == rec["sum_inside"][0, c]
        assert [int(w[4]), int(w[5]), int(w[6])] == [rec["n_inside"][0, c], rec["flags"][0, c], edge[0, c]]
    assert edge[0, 2] >= 224 and edge[0, 0] == 0
