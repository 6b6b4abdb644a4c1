"""hd_m_expm1_neg (pyharp_amd/csrc/hd_device.hpp) on the CPU: tests/cpp/expm1_check.cpp,
compiled with g++ here from the header's host build, holds 1 - exp(-x) within 4 ulp of
expm1 of long double at x = 0, denormal x, 1e-300, 2 000 points log-spaced in [1e-12, 800],
the doubles around every n ln2 (n = 1 .. 64) and every (n + 1/2) ln2, 745, 1e4 and +inf.
Measured maximum: 1.100 ulp (at x = 0.3595)."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_expm1_check(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "expm1_check.cpp")
    exe = str(tmp_path / "expm1_check")
    # -ffp-contract=off: the program's own arithmetic as written; the helper asks for its
    # FMAs by name
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", src,
            "-o", exe]
    # under the address and undefined-behaviour sanitizers where g++ has their runtimes
    # (a stand-alone program: nothing is preloaded); plain otherwise
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout[-2000:])
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert "expm1_check: ok" in res.stdout
