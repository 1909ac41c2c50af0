"""The upload block of the operator-level keyframe calls (cuahn_vio_amd/csrc/keyframe_upload.h; hnet_op_keyframe_render, _localise, _adjust and
_adjust_solve) on the CPU: the stand-alone program tests/cpp/keyframe_upload_check.cpp under AddressSanitizer + UBSan walks every m in 1 .. 8 and every
combination of the optional sections - alignment, order without overlap, inside the total - and pins the layouts of the four calls to the offsets they
computed by hand before the header existed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keyframe_upload_check_under_asan_ubsan(tmp_path):
    """a stand-alone program; nothing loaded into python is sanitized"""
    exe = str(tmp_path / "keyframe_upload_check_san.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "keyframe_upload_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "keyframe_upload_check: ok (192 layouts)" in r.stdout
