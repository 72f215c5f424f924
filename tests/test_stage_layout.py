"""The buffer plans of the five batched solvers and the helpers of orb_slam2_2021_amd/csrc/orbfe_stage.h in a
stand-alone program built with ASan + UBSan (tests/cpp/stage_layout_test.cpp); CPU only, no library. Each solver
has one layout function that both sizes its handle's buffers (over counting blocks) and places a solve (over the
real ones). The program lays every plan out over heap buffers of exactly the counted size and writes every byte
of every region, holds the sizes at a handle's bounds to the closed formulas restated by hand and every offset to
the restated take order, and checks ransac_max_its, ransac_check_draws and orbfe_unpack_masks at their edges."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def exe():
    out_dir = os.path.join(CPP, "build")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "stage_layout_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(CPP, "hipstub"), "-o", path,
                    os.path.join(CPP, "stage_layout_test.cpp")], check=True)
    return path


def test_plans_sizes_offsets_and_helpers(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.startswith("stage_layout_test: ok, "), out.stdout[-2000:]
    assert int(out.stdout.split()[2]) > 10000  # the walk ran: thousands of regions, each checked
