"""CPU: the lane network of the reference-side credit (clustering_amd/csrc/dc_credit.hpp) on 64 emulated
lanes.  tests/cpp/test_credit_model.cpp instantiates the header's own credit_slots / credit_network -- the text the
kernels compile -- over arrays, with exchanges written from the ISA's description of the DPP controls and of
v_permlane16_swap, and compares every crediting lane with a plain column sum over the 32 lanes of its half-wave:

  binary   all 2^16 patterns of elements at count 0 or 6, in every lane at once (among them all 32 x 16 counts at 6: every
           sum 192) and in one lane per half at a time; every (lane, element) alone
  random   300 000 seeded inputs with counts 0 .. 6 per (lane, element)
  bounds   no field above its level's bound (6, 12, 24, 48, 96, 192) at any level of any input, each bound within its field
  rows     16 crediting lanes per half-wave; each of the 32 rows of a tile is credited by exactly one lane, the row
           tile_row names for the element that lane holds

What the model cannot see is whether the hardware's exchanges do what the ISA text says; tests/test_gpu_credit.py holds
the kernels to the oracle on a device."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_credit_model.cpp")
INC = os.path.join(ROOT, "clustering_amd", "csrc")
N_RANDOM = 300000


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the credit model is a host program: g++ is needed"
    exe = str(tmp_path_factory.mktemp("credit") / "test_credit_model")
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-I", INC, "-o", exe, SRC],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, str(N_RANDOM)], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    words = r.stdout.split()
    assert words and words[0] == "binary", r.stdout[-2000:] + r.stderr[-2000:]
    figures = {words[i]: int(words[i + 1]) for i in range(0, 10, 2)}
    figures["level_max"] = [int(w) for w in words[11:17]]
    figures["returncode"] = r.returncode
    figures["ok"] = r.stdout.strip().endswith("OK")
    return figures


def test_sums_match_the_column_sums(model):
    assert model["binary"] == 3 * 65536 + 32 * 16
    assert model["random"] == N_RANDOM
    assert model["mismatches"] == 0


def test_no_field_exceeds_its_bound(model):
    assert model["bound_failures"] == 0
    # the saturating input reaches every bound, so the bounds are tight and the check above is not vacuous
    assert model["level_max"] == [6, 12, 24, 48, 96, 192]


def test_every_row_is_credited_by_one_lane(model):
    assert model["row_failures"] == 0


def test_model_verdict(model):
    assert model["returncode"] == 0 and model["ok"]
