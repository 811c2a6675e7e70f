"""CPU-side checks of the nearest-interval query (bivx_nearest*, include/bivx.h): declared and exported, bound in
binary_amd/capi.py, its kernels free of scratch, and the C++ facade's find_nearest compiles for 32- and 64-bit keys."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from binary_amd import _build, capi
    _build.build_lib()
    return capi.load()


def test_nearest_entry_points_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bivx.h")).read(), flags=re.S)
    from binary_amd import capi
    for name in ("bivx_nearest", "bivx_nearest_dev"):
        assert re.search(rf"\bint {name}\s*\(", text), f"{name} is not declared in include/bivx.h"
        assert hasattr(lib, name), f"libbivx.so does not export {name}"
        assert name in capi.EXPORTS
    assert lib.bivx_nearest.argtypes is not None and len(lib.bivx_nearest.argtypes) == 9
    assert lib.bivx_nearest_dev.argtypes is not None and len(lib.bivx_nearest_dev.argtypes) == 10


def test_nearest_kernels_have_no_scratch():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    ru = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ru)
    assert "nearest.hip" in ru.DEFAULT  # (so that test_capi_cpu.py::test_no_kernel_spills_to_scratch covers them)
    rows = [r for r in ru.usage(("nearest.hip",)) if "k_nearest" in r["name"]]
    assert len(rows) == 2, rows
    for r in rows:
        assert r["scratch"] == 0, r
        assert r["vgpr"] <= 64 and r["occupancy"] == 8, r


def test_facade_find_nearest_compiles(tmp_path):
    from binary_amd import _build
    _build.build_lib()
    src = tmp_path / "find_nearest.cpp"
    src.write_text("""
#include <binary/algorithm/all.hpp>
#include <cstdint>
using namespace binary::algorithm::tree;
int main() {
  IntervalTree<UIntIntervalNode> a{0};
  IntervalTree<IntervalNode<BaseInterval<std::int64_t>>> b{0};
  std::optional<UIntInterval> x = a.find_nearest(UIntInterval{5u, 6u});
  std::optional<UIntInterval> y = a.find_nearest(UIntInterval{5u, 6u}, 3u);
  auto z = b.find_nearest(BaseInterval<std::int64_t>{-5, 6});
  auto w = b.find_nearest(BaseInterval<std::int64_t>{5, 6}, std::int64_t{7'000'000'000});
  return x.has_value() + y.has_value() + z.has_value() + w.has_value();
}
""")
    libdir = os.path.join(ROOT, "binary_amd")
    for f in (str(src), os.path.join(ROOT, "tests", "cpp", "facade_nearest.cpp")):
        r = subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                            f, "-o", str(tmp_path / "a.out"), "-L", libdir, "-lbivx", "-pthread",
                            f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
