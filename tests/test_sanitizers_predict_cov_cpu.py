"""CPU: the covariance additions of include/hnet_ekf.h (odometry_cov_from_state, propagate_jacobians_fill) and the host restatement of
hnet_filters_predict_cov under AddressSanitizer + UndefinedBehaviorSanitizer, built the way tests/test_sanitizers_predict_cpu.py builds host code.
The program is tests/cpp/filters_predict_cov_ref.cpp with its own main: windows of 0 .. 41 intervals with imu_avg on and off, an empty history and a
history of one reading, the fill split on buffers zeroed once against the body before the split, the batch form on threads."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_predict_cov_header_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "filters_predict_cov_check_san.bin")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", *SAN, "-pthread", "-DPREDICT_COV_CHECK_MAIN", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_predict_cov_ref.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "predict_cov check: 6 propagated cases moved the covariance, statuses ok 8 wait 4" in r.stdout, r.stdout
