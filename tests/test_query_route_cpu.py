"""The single-pass route policy (binary_amd/csrc/query_route.h): tests/cpp/query_route.cpp compiles the header alone with
g++ -std=c++17 (no HIP, no GPU) and checks the route, launch sizes and in-kernel ordering at each threshold, and how the
environment knobs are parsed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_route_policy(tmp_path):
    exe = str(tmp_path / "query_route")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "binary_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "query_route.cpp"),
                    "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
