"""pyharp_amd/csrc/hd_plan.hpp on the CPU: tests/cpp/plan_check.cpp, compiled with g++
here, checks the scratch layout of the flux solves (regions non-empty where used, aligned
where the kernels read pairs, disjoint, inside the total, the total equal to the sizes the
solve and hd_context_reserve used to compute by hand), that a reserved context covers every
smaller automatically chunked call on both band routes, and the automatic chunk sizes."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_check(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "plan_check.cpp")
    exe = str(tmp_path / "plan_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", src, "-o", exe]
    # under the address and undefined-behaviour sanitizers where g++ has their runtimes
    # (a stand-alone program: nothing is preloaded); plain otherwise
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert "plan_check: ok" in res.stdout
