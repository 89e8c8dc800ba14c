"""The kernel-variant rule and render()'s launch plan on the CPU (no GPU): tests/native/launch_plan_host.cpp includes
only csrc/vpt_variant.h and checks that the variant index round-trips over all 1 024 flag combinations, that
variant_valid holds for exactly the library's 45 integrate kernels, and that plan_launch / attachments_refuse reproduce
every row of tests/golden/launch_plans.json -- the decisions render() made when they were still written out in it
(EXPERIMENTS.md says how the rows were made).  Built as a plain program with the host C++ compiler (no HIP in it; the
one tests/native/Makefile builds run_gpu_harness with), once more under AddressSanitizer + UBSan."""
import os
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SOURCE = ROOT / "tests" / "native" / "launch_plan_host.cpp"
GOLDEN = ROOT / "tests" / "golden" / "launch_plans.json"
CXX = os.environ.get("CXX", "g++")


@pytest.mark.parametrize("sanitize", [False, True])
def test_launch_plan_host_program(tmp_path, sanitize):
    flags = (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
             if sanitize else ["-O2"])
    exe = tmp_path / "launch_plan_host"
    r = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), str(SOURCE)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe), str(GOLDEN)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "launch_plan_host ok" in r.stdout and "FAIL" not in r.stdout
    assert "variants 45 of 1024" in r.stdout
    rows, refused, variants = map(int, re.search(r"rows (\d+) refused (\d+) variants (\d+)", r.stdout).groups())
    # every integrate kernel but the three gang ones (which render() never plans) is some row's plan
    assert rows >= 300 and 0 < refused < rows and variants == 42
    assert GOLDEN.stat().st_size < 100 * 1024
