"""The direct-addressed stencil pool, host side (no GPU): tests/native/dense_pool_host.cpp runs the __host__
__device__ functions the kernels call -- dense_square (the expansion), dense_index and trilinear's dense path --
against cell_at / fetch_stencil / the sparse path, bit for bit, on the 64^3 cloud, the fire temperature stand-in,
the constant cube and the sparse anchor grid (leaves, active and inactive lower tiles, an upper tile, a root tile,
empty space).  Built like band_host.cpp (hipcc, host only) as a plain program, once more under AddressSanitizer +
UBSan: the sanitizer run of the new index arithmetic."""
import re
import subprocess

import pytest

import dense_pool_lib as DP
import grids as G
from volume_path_tracer_amd.scenes import SynthGrid


def host_grids():
    return {"cloud64": SynthGrid(1, 64).grid(copy=True), "fire_temperature64": SynthGrid(2, 64).grid(copy=True),
            "cube128": SynthGrid(0, 128).grid(copy=True), "sparse_anchor": G.sparse_grid()}


@pytest.fixture(scope="module")
def grid_files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dense_pool_host")
    return tmp, [DP.write_grid(tmp / (name + ".grid"), g) for name, g in host_grids().items()]


@pytest.mark.parametrize("sanitize", [False, True])
def test_dense_pool_host_program(grid_files, sanitize):
    """Every cell of the cells8 table, every voxel: the dense stencil's eight floats are fetch_stencil's through
    cell_at (uint32) -- the table's last rows, whose +1 apron lies outside it, included; a leaf's copied brick is what
    dense_square computes; trilinear dense and sparse agree in value bits and refresh flag at points inside, around
    and far outside the table, alone and along walks that share a StencilCell."""
    tmp, files = grid_files
    if sanitize:
        exe = DP.compile_program(tmp / "dense_pool_host_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    else:
        exe = DP.build_program()
    r = subprocess.run([str(exe), *map(str, files)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "dense_pool_host ok" in r.stdout and "FAIL" not in r.stdout
    rows = re.findall(r"cells (\d+) leaves (\d+) stencils (\d+) points (\d+)", r.stdout)
    assert len(rows) == len(files)
    for cells, leaves, stencils, points in rows:
        assert int(stencils) == int(cells) * 512 and int(points) > 100000
    # the anchor grid's table spans its five lower nodes' bounding box; the others one lower node
    assert [int(c) for c, *_ in rows] == [16 ** 3, 16 ** 3, 16 ** 3, 80 * 80 * 48]
    assert all(int(r[1]) > 0 for r in rows)
