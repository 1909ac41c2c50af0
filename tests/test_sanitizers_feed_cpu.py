"""CPU: the cold-start additions of include/hnet_ekf.h (initialize_with_imu, initialize_cov, the retention rules, select_span + select_imu_readings on
the span) under AddressSanitizer + UndefinedBehaviorSanitizer, built the way tests/test_sanitizers_cpu.py builds host code.  The program is
tests/cpp/filters_feed_ref.cpp with its own main: the streams of the initialiser's cases (one-reading windows and an empty history among them) and
400 random windows over histories with repeated stamps, where the span's selection must equal the whole history's byte for byte."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_feed_header_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "filters_feed_check_san.bin")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", *SAN, "-DFEED_CHECK_MAIN", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_feed_ref.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "feed check: accepted 2 refused 4" in r.stdout, r.stdout
