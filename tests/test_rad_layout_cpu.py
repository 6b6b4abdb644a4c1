"""The intensity path's layouts and Y_l^m table fill (pyharp_amd/csrc/hd_rad_layout.hpp) on
the CPU: tests/cpp/rad_layout_check.cpp, compiled with g++ here from the header itself (it
needs no HIP).  For nn = 1..16: every record's fields contiguous, in the documented order,
sizes equal to the counts written out in the program, the user-angle maps inside the records
they overwrite, both addressings a bijection; the table at the double-Gauss nodes against
Bonnet's recurrence in long double and the addition theorem, absolute tolerance 5e-13."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rad_layout_check(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "rad_layout_check.cpp")
    exe = str(tmp_path / "rad_layout_check")
    # -ffp-contract=off: the header's recurrence as written
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
            "-I", os.path.join(ROOT, "pyharp_amd", "csrc"), src, "-o", exe]
    # under the address and undefined-behaviour sanitizers where g++ has their runtimes
    # (a stand-alone program: nothing is preloaded); plain otherwise
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout[-2000:])
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert "rad_layout_check: ok" in res.stdout
