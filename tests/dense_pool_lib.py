"""tests/native/dense_pool_host.cpp as a program: the direct-addressed stencil pool's expansion and lookups on the
CPU.  Compiled with hipcc, host only, like tests/alpha_lib.py compiles matte_host.cpp (tests/native/Makefile does not
know it): on first use, or ahead of the tests by __graft_entry__.build()."""
from __future__ import annotations

import os
import struct
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
NATIVE = ROOT / "tests" / "native"
CSRC = ROOT / "volume_path_tracer_amd" / "csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = [NATIVE / "dense_pool_host.cpp", CSRC / "vpt_scene.cpp", CSRC / "vpt_grid_build.cpp", CSRC / "vpt_config.cpp"]
# hostsim's float flags (tests/native/Makefile): no contraction, the device's semantics on the host
FLAGS = ["-std=c++20", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "--cuda-host-only", "-pthread",
         "-I" + str(ROOT / "include")]
PROGRAM = NATIVE / "build" / "dense_pool_host"
BRICK_FLOATS = 2304  # kBrickVox: [y 8][z 8][x 9][4]


def compile_program(out: Path, extra=("-O2",)) -> Path:
    out.parent.mkdir(parents=True, exist_ok=True)
    r = subprocess.run([HIPCC, *FLAGS, *extra, "-o", str(out), *map(str, SOURCES)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def build_program() -> Path:
    """The optimised program, rebuilt when a source or header is newer (__graft_entry__.build() calls this too, so
    the tests of a built tree compile only the sanitizer build)."""
    deps = SOURCES + sorted(CSRC.glob("*.h")) + [ROOT / "include" / "vpt_gpu.h"]
    if not PROGRAM.exists() or PROGRAM.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        tmp = PROGRAM.with_name(f"{PROGRAM.name}.{os.getpid()}.tmp")
        compile_program(tmp)
        os.replace(tmp, PROGRAM)
    return PROGRAM


def write_grid(path: Path, g) -> Path:
    """The file dense_pool_host.cpp's read_grid reads: counts, map, bbox, then vpt_grid_desc's arrays."""
    d = g.desc
    nt = 0 if g.tile_origin is None else g.tile_origin.shape[0]
    nl = 0 if g.lower_origin is None else g.lower_origin.shape[0]
    nu = 0 if g.upper_origin is None else g.upper_origin.shape[0]
    with open(path, "wb") as f:
        f.write(struct.pack("<4Q", g.leaf_count, nt, nl, nu))
        f.write(np.asarray(list(d.map_mat) + list(d.map_inv_mat) + list(d.map_vec) + [d.background], np.float32).tobytes())
        f.write(np.asarray(list(d.index_bbox_min) + list(d.index_bbox_max), np.int32).tobytes())
        for a in (g.leaf_origin, g.leaf_values, g.leaf_value_mask, g.leaf_max):
            f.write(a.tobytes())
        if nt:
            for a in (g.tile_origin, g.tile_level, g.tile_value, g.tile_active):
                f.write(a.tobytes())
        if nl:
            f.write(g.lower_origin.tobytes())
        if nu:
            f.write(g.upper_origin.tobytes())
    return path


def host_bricks(grid_file: Path, cell_begin: int, cell_count: int, tmp: Path) -> np.ndarray:
    """The host expansion of table cells [cell_begin, + cell_count): float32 [cell_count][2304]."""
    out = tmp / f"bricks_{cell_begin}_{cell_count}.bin"
    r = subprocess.run([str(build_program()), str(grid_file), "--dump", str(cell_begin), str(cell_count), str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return np.fromfile(out, np.float32).reshape(cell_count, BRICK_FLOATS)
