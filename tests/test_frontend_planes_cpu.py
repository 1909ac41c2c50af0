"""CPU: tests/frontend_planes.py (the numpy form of split2h / join2h / split3 the GPU front-end tests compare the block-4 planes with) against
csrc/s3_format.h itself, compiled host-only, bit for bit on a fixed value list; and the plane-layout constants of _capi.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import frontend_planes as fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_numpy_planes_are_the_bits_of_s3_format_h(tmp_path):
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        clang = shutil.which("hipcc")
    if not clang:
        pytest.skip("no HIP compiler on this machine (the header includes hip_runtime.h)")
    vals = fp.plane_test_values()
    assert vals.size > 800 and (vals == 0).sum() == 3 and (vals < 0).any() and (vals > 1).any() and ((vals > 0) & (vals < 2.0 ** -14)).sum() > 64
    src = tmp_path / "values.txt"
    src.write_text("".join(f"{int(b):08x}\n" for b in vals.view(np.uint32)))
    out = str(tmp_path / "frontend_planes_print.bin")
    subprocess.run([clang, "-O2", "-x", "hip", "--offload-host-only", "-I" + ROOT, "-I/opt/rocm/include", "-w",
                    os.path.join(ROOT, "tests", "cpp", "frontend_planes_print.cpp"), "-o", out], check=True, timeout=300)
    r = subprocess.run([out, str(src)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = np.array([[int(t, 16) for t in line.split()] for line in r.stdout.splitlines()], np.uint64)
    assert rows.shape == (vals.size, 8) and np.array_equal(rows[:, 0], vals.view(np.uint32))
    a0, a1 = fp.split2h(vals)
    b0, b1, b2 = fp.split3(vals)
    got = {"split2h.A0": a0, "split2h.A1": a1, "join2h": fp.join2h(a0, a1).view(np.uint32), "split3.a": b0, "split3.b": b1, "split3.c": b2,
           "join3": fp.join3(b0, b1, b2).view(np.uint32)}
    for col, (name, g) in enumerate(got.items(), start=1):
        bad = np.flatnonzero(g.astype(np.uint64) != rows[:, col])
        assert bad.size == 0, (name, [(float(vals[i]), hex(int(g[i])), hex(int(rows[i, col]))) for i in bad[:5]])
    # what the formats promise on this list: the bf16 split is exact (above 2^-110: three 8-bit planes of a value whose last bit is still a bf16
    # number); the fp16 split is exact to fp32's last bit inside the fp16 range
    big = (np.abs(vals) >= 2.0 ** -110) | (vals == 0)
    assert np.array_equal(fp.join3(b0, b1, b2)[big], vals[big]) and (~big).sum() == 1
    unit = (np.abs(vals) <= 1.0) & (np.abs(vals) >= 2.0 ** -14)
    assert np.abs(fp.join2h(a0, a1)[unit].astype(np.float64) - vals[unit]).max() <= 2.0 ** -24
    # the dword of a pixel: low half img1, high half the warped img2
    assert fp.pack(np.array([0x1234], np.uint16), np.array([0xABCD], np.uint16))[0] == 0xABCD1234


def test_expected_planes_layout():
    x = np.zeros((2, 2, 224, 320), np.float32)
    x[1, 0, 3, 7], x[1, 1, 3, 7] = 0.5, 1.0
    for n_planes, lo, hi in ((2, 0x3800, 0x3C00), (3, 0x3F00, 0x3F80)):
        d, j = fp.expected_planes(x, n_planes)
        assert d.shape == (n_planes, 2, 224, 320) and d.dtype == np.uint32 and j.shape == x.shape
        assert d[0, 1, 3, 7] == (hi << 16 | lo) and not d[1:].any() and np.count_nonzero(d) == 1 and np.array_equal(j, x)


def test_capi_plane_constants_are_pinned_by_the_static_asserts():
    """_capi.B4_* are the numbers tests/cpp/b41_tap_check.cpp static_asserts against csrc/kernels.h (compiled by tests/test_s3_format_host.py)"""
    import re
    from cuahn_vio_amd import _capi
    txt = open(os.path.join(ROOT, "tests", "cpp", "b41_tap_check.cpp")).read()
    m = re.search(r"B4_HP == (\d+) && B4_WP == (\d+) && B4_PADX == (\d+) && B4_PADY == (\d+)", txt)
    assert m and tuple(int(v) for v in m.groups()) == (_capi.B4_HP, _capi.B4_WP, _capi.B4_PADX, _capi.B4_PADY)
    assert _capi.B4_HP >= 224 + 2 * _capi.B4_PADY and _capi.B4_WP >= 320 + 2 * _capi.B4_PADX and _capi.B4_SENTINEL == 0xA5A5A5A5
