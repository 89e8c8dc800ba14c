#!/usr/bin/env python3
"""Writes tests/golden/matte_planes.npz from the host build of the matte march (csrc/vpt_alpha.h, vpt_depth.h, bound by
tests/alpha_lib.py and tests/depth_lib.py), to freeze its bits: the GPU tests hold vpt_alpha_kernel and
vpt_depth_kernel to that host build byte for byte, so an edit of the march that moves a bit in both would pass them;
it shows up against this file (tests/test_matte_golden.py).

    python tools/make_golden_matte.py

Per frame <s> of SCENES: "<s>_tau" the matte's tau plane float32 [H][W], "<s>_depth" and "<s>_reach" float32 [K][H][W],
and "<s>_upto" the march cut (vptd_tau_upto) at the level-1 depth of every pixel that reached level 1, in row-major
order: the finite-cut path.  The alpha plane is left out: its expf is the platform's.
From the stand-alone program's fixed ray table, per volume of VOLUMES: "prog_tau" float32 [4][rays], "prog_reached"
uint32 [4][rays] and "prog_z" float32 [4][rays][4], +0.0 for the levels a ray did not reach (%.9g prints an fp32
exactly).
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import alpha_lib as AL  # noqa: E402
import analytic_anchor as A  # noqa: E402
import depth_lib as DL  # noqa: E402
from test_analytic_sparse import camera_config  # noqa: E402
from test_depth_host import LEVELS, cube_config, sparse_cfg  # noqa: E402
from volume_path_tracer_amd.scenes import SynthGrid, workload  # noqa: E402

FOUR = (0.25, 0.5, float(np.float32(0.5) + np.float32(1e-6)), 0.9)  # two levels that land in one piece
SCENES = ("cube", "anchor", "cloud", "fire")
VOLUMES = ("cloud", "cube", "voxel 2^-20", "voxel 2^27")


def scene(name):
    """(cfg, density grid, opacity levels, sub-rays per axis) of a frame."""
    if name == "cube":
        return cube_config(), SynthGrid(0, 128).grid(), LEVELS, 1
    if name == "anchor":
        return sparse_cfg(), A.anchor_grid(), LEVELS, 1
    if name == "cloud":  # 37x21, jitter on: ragged tiles, two levels in one piece, partial reach
        cfg = camera_config(True).cfg
        cfg.output_size[0], cfg.output_size[1] = 37, 21
        cfg.tile_size[0], cfg.tile_size[1] = 8, 8
        return cfg, SynthGrid(1, 64).grid(), FOUR, 2
    if name == "fire":
        return workload("c4", width=24, height=24, spp=1, grid_n=64).cfg, SynthGrid(1, 64).grid(), LEVELS, 1
    raise KeyError(name)


def golden_planes(name):
    cfg, g, levels, sub = scene(name)
    _, tau = AL.render(cfg, g, sub)
    depth, reach = DL.render(cfg, g, levels, sub)
    ys, xs = np.nonzero(depth[1] > 0)
    upto = DL.tau_upto(cfg, g, xs, ys, depth[1][ys, xs])
    return {f"{name}_tau": tau, f"{name}_depth": depth, f"{name}_reach": reach, f"{name}_upto": upto}


def _run(mod, macro, tmp):
    exe = mod.compile_host(Path(tmp) / macro.lower(), ["-O2", "-D" + macro])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def golden_program():
    """The stand-alone program's rays (the alpha program's and the depth program's output, one program or two)."""
    with tempfile.TemporaryDirectory() as tmp:
        out = _run(AL, "ALPHA_HOST_MAIN", tmp)
        if "reached" not in out:
            out += _run(DL, "DEPTH_HOST_MAIN", tmp)
    num = r"([-+.\w]+)"
    tau, got, z = [], [], []
    for v in VOLUMES:
        t = re.findall(r"^%s ray \d+: tau %s$" % (re.escape(v), num), out, re.M)
        d = re.findall(r"^%s ray \d+: reached (\d) z %s %s %s %s$" % (re.escape(v), num, num, num, num), out, re.M)
        assert len(t) == len(d) > 0, (v, len(t), len(d))
        tau.append([float(x) for x in t])
        got.append([int(row[0]) for row in d])
        z.append([[float(x) if k < int(row[0]) else 0.0 for k, x in enumerate(row[1:])] for row in d])
    return {"prog_tau": np.asarray(tau, np.float32), "prog_reached": np.asarray(got, np.uint32),
            "prog_z": np.asarray(z, np.float32)}


def golden():
    out = golden_program()
    for name in SCENES:
        out.update(golden_planes(name))
    return out


def main():
    path = ROOT / "tests" / "golden" / "matte_planes.npz"
    np.savez_compressed(path, **golden())
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
