"""The block-envelope LDL^T shared by the global bundle adjuster and the essential-graph optimizer
(orb_slam2_2021_amd/csrc/orbfe_env_core.h) against the scalar rule, bit for bit, for block dimensions 6 and
7, its structure pass and its failing pivots, in a stand-alone program built with ASan + UBSan; CPU only
(tests/cpp/env_core_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_env_core_under_sanitizers(tmp_path):
    exe = str(tmp_path / "env_core_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(CPP, "env_core_test.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK envelope core"), out.stdout
