"""BeerGradPlan (pyharp_amd/csrc/hd_plan.hpp) on the CPU: tests/cpp/beer_grad_plan_check.cpp,
compiled with g++ here, checks the scratch layout of the Beer-Lambert gradient calls
(regions disjoint, in the documented order, filling the total) and the chunk size under
the caller's bound, the automatic bound and the 16 GB budget."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_beer_grad_plan_check(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "beer_grad_plan_check.cpp")
    exe = str(tmp_path / "beer_grad_plan_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", src, "-o", exe]
    # under the address and undefined-behaviour sanitizers where g++ has their runtimes
    # (a stand-alone program: nothing is preloaded); plain otherwise
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert "beer_grad_plan_check: ok" in res.stdout
