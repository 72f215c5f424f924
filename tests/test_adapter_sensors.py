"""adapter/Frame_sensors_gpu.cc (Frame::UndistortKeyPoints, ComputeImageBounds, ComputeStereoFromRGBD) compiled over
the test-only declarations -- tests/cpp/cvstub_sensors/ before tests/cpp/cvstub/ on the include path, so the superset
Frame.h with mDistCoef is found first and the existing stubs stay as they are -- and run on one frame against the
host entry points of include/orbfe_frame.h (tests/cpp/adapter_sensors_test.cpp). CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def exe():
    from orb_slam2_2021_amd import _lib as L
    L.lib()  # the library is built
    out_dir = os.path.join(CPP, "build")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "adapter_sensors_test")
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-I" + os.path.join(CPP, "cvstub_sensors"), "-I" + os.path.join(CPP, "cvstub"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"), "-o", path,
                    os.path.join(CPP, "adapter_sensors_test.cpp"), os.path.join(ROOT, "adapter", "Frame_sensors_gpu.cc"),
                    "-L" + lib_dir, "-lorbfe", "-Wl,-rpath," + lib_dir], check=True)
    return path


def test_adapter_bodies_reproduce_the_host_entry_points(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "adapter_sensors_test OK" in out.stdout
    assert out.stdout.count(" moved, ") == 2  # 4 and 5 coefficients


def test_the_adapter_is_empty_outside_the_reference_tree(tmp_path):
    # without Frame.h on the include path the translation unit compiles to nothing (the __has_include guard)
    obj = tmp_path / "empty.o"
    subprocess.run(["g++", "-std=c++17", "-c", "-I" + os.path.join(ROOT, "include"), "-o", str(obj),
                    os.path.join(ROOT, "adapter", "Frame_sensors_gpu.cc")], check=True)
    syms = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    assert "Frame" not in syms
