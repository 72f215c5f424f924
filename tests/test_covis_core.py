"""The covisibility table's host bookkeeping (orb_slam2_2021_amd/csrc/orbfe_covis_core.h: id table, row reuse,
tie-key and mnId ranks, stale tracking, argument and capacity checks) in a stand-alone program built with
ASan + UBSan; CPU only (tests/cpp/covis_core_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_covis_core_under_sanitizers():
    out_dir = os.path.join(CPP, "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "covis_core_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(CPP, "covis_core_test.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK covisibility core"), out.stdout
    # the host figure's generator on a toy shape, under the sanitizers as well
    out = subprocess.run([exe, "--bench", "12", "40", "4", "3", "1"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and '"host_update_connections_ms"' in out.stdout, out.stdout + out.stderr
