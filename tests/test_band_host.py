"""Tile-band launches, host side (no GPU): the cost-balanced band partition of the multi-GPU `bands` mode
(distributed.cost_bands / rank_tile_band: the cuts of include/vpt_run.hpp's detail::cost_bands), the band launch's
item -> (tile, wave) mapping and lane-adjacent sample layout (tests/native/band_host.cpp runs the __host__
__device__ functions the kernels call, also under AddressSanitizer + UBSan as a plain program), and the ABI entry
vpt_gpu_render_tiles."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from volume_path_tracer_amd import capi
from volume_path_tracer_amd import distributed as D

ROOT = Path(__file__).resolve().parents[1]
NATIVE = ROOT / "tests" / "native"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# hostsim's flags (tests/native/Makefile) with C++20 for vpt_run.hpp, and its include paths
FLAGS = ["-O1", "-g", "-std=c++20", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "--cuda-host-only",
         "-I" + str(ROOT / "include")]


def _cost_vectors():
    rng = np.random.default_rng(20)
    one_hot = np.zeros(40, np.float32)
    one_hot[17] = 5.0
    return {
        "uniform": np.full(30, 2.5, np.float32),
        "one_hot": one_hot,
        "all_zero": np.zeros(24, np.float32),
        "random": rng.gamma(0.7, 40.0, 97).astype(np.float32),
        "random_with_negatives": (rng.standard_normal(33) * 10).astype(np.float32),
        "eight": np.arange(8, dtype=np.float32)[::-1].copy(),  # T == 8: single-tile bands for world 8
    }


WORLDS = (1, 2, 3, 8)


@pytest.mark.parametrize("name", list(_cost_vectors()))
@pytest.mark.parametrize("world", WORLDS)
def test_cost_bands_partition(name, world):
    cost = _cost_vectors()[name]
    T = len(cost)
    cut = D.cost_bands(cost, world)
    assert len(cut) == world + 1 and cut[0] == 0 and cut[-1] == T
    assert all(b > a for a, b in zip(cut[:-1], cut[1:])), cut  # monotone, non-empty
    bands = [D.rank_tile_band(r, world, cost) for r in range(world)]
    assert bands == list(zip(cut[:-1], cut[1:]))
    covered = np.zeros(T, int)
    for lo, hi in bands:
        covered[lo:hi] += 1
    assert (covered == 1).all()
    if T == world:
        assert cut == list(range(T + 1))


def test_cost_bands_balance_and_errors():
    # equal costs: equal bands; one costly tile ends its band
    assert D.cost_bands(np.ones(12, np.float32), 3) == [0, 4, 8, 12]
    assert D.cost_bands(np.ones(12, np.float32), 1) == [0, 12]
    assert D.cost_bands([1, 1, 1, 1], 4) == [0, 1, 2, 3, 4]
    cut = D.cost_bands(np.array([1, 1, 100, 1, 1, 1], np.float32), 2)
    assert cut == [0, 2, 6]  # (the goal, 52.5, is passed inside tile 2: the cut stays before it)
    with pytest.raises(ValueError):
        D.cost_bands(np.ones(3, np.float32), 4)
    with pytest.raises(ValueError):
        D.rank_tile_band(0, 5, np.ones(4, np.float32))
    with pytest.raises(ValueError):
        D.rank_tile_band(2, 2, np.ones(4, np.float32))
    assert D.total_samples_per_pixel(4, 16, "bands") == 16


def _build(tmp, name, extra):
    exe = tmp / name
    r = subprocess.run([HIPCC, *FLAGS, *extra, "-o", str(exe), str(NATIVE / "band_host.cpp")], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def costs_file(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("band_host")
    lines, expect = [], []
    for cost in _cost_vectors().values():
        for world in WORLDS:
            if len(cost) < world:
                continue
            lines.append(" ".join([str(world)] + ["%.9g" % float(v) for v in cost]))
            expect.append(D.cost_bands(cost, world))
    (tmp / "costs.txt").write_text("\n".join(lines) + "\n")
    return tmp, expect


@pytest.mark.parametrize("sanitize", [False, True])
def test_band_host_program(costs_file, sanitize):
    """The mapping is a bijection onto the band's jobs, the slots are unique, in range and lane-adjacent (the
    program's own checks, for (T, tile_lo, tile_hi, n) in {(30,7,19,6), (20,3,20,5), (30,0,30,66), (30,29,30,130)}),
    and vpt_run.hpp's cost_bands prints the cuts distributed.cost_bands computes.  Once more as an
    AddressSanitizer + UBSan build, run directly."""
    tmp, expect = costs_file
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else []
    exe = _build(tmp, "band_host_san" if sanitize else "band_host", extra)
    r = subprocess.run([str(exe), str(tmp / "costs.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "band_host ok" in r.stdout and "FAIL" not in r.stdout
    cuts = [[int(v) for v in m.split()] for m in re.findall(r"^cuts:(.*)$", r.stdout, re.M)]
    assert cuts == expect


def test_render_tiles_abi():
    lib = capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True, text=True).stdout
    assert re.search(r"\bT vpt_gpu_render_tiles\b", out)
    VPT_E_INVALID = 1
    header = (ROOT / "include" / "vpt_gpu.h").read_text()
    assert re.search(r"VPT_E_INVALID\s*=\s*1\b", header), "VPT_E_INVALID moved"
    assert lib.vpt_gpu_render_tiles(None, 0, 1, 0, 1, None, None) == VPT_E_INVALID
    assert b"null context" in lib.vpt_last_error()
    assert lib.vpt_abi_version() == 1
    assert lib.vpt_gpu_render_tiles.argtypes[1] is C.c_uint32
