"""ctypes binding of tests/native/matte_host.cpp, the coverage pass's part: the march of csrc/vpt_alpha.h (the code
vpt_alpha_kernel runs per lane) on the CPU.  tests/depth_lib.py binds the depth pass's part of the same library.  It is
compiled here, once for both, with hipcc, host only, like tests/test_band_host.py compiles band_host.cpp
(tests/native/Makefile does not know it): on first use, or ahead of the tests by __graft_entry__.build()."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

from volume_path_tracer_amd.capi import Configuration, GridDesc

ROOT = Path(__file__).resolve().parents[1]
NATIVE = ROOT / "tests" / "native"
CSRC = ROOT / "volume_path_tracer_amd" / "csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = [NATIVE / "matte_host.cpp", CSRC / "vpt_scene.cpp", CSRC / "vpt_grid_build.cpp", CSRC / "vpt_config.cpp"]
# hostsim's float flags (tests/native/Makefile): no contraction, the device's semantics on the host
FLAGS = ["-std=c++20", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "--cuda-host-only",
         "-I" + str(ROOT / "include")]
LIB = NATIVE / "build" / "libvpt_matte_host.so"
_L = None


def compile_host(out: Path, extra=()) -> Path:
    """hipcc, host only: the library (extra = ["-O2", "-shared"]) or the stand-alone program (-DALPHA_HOST_MAIN or
    -DDEPTH_HOST_MAIN: one program, both marches)."""
    out.parent.mkdir(parents=True, exist_ok=True)
    r = subprocess.run([HIPCC, *FLAGS, *extra, "-o", str(out), *map(str, SOURCES)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def build_lib() -> Path:
    """The shared library, rebuilt when a source or header is newer (__graft_entry__.build() calls this too, so the
    tests of a built tree compile nothing)."""
    deps = SOURCES + sorted(CSRC.glob("*.h")) + [ROOT / "include" / "vpt_gpu.h"]
    if not LIB.exists() or LIB.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        tmp = LIB.with_name(f"{LIB.name}.{os.getpid()}.tmp")
        compile_host(tmp, ["-O2", "-shared"])
        os.replace(tmp, LIB)
    return LIB


def lib():
    global _L
    if _L is None:
        build_lib()
        import torch  # noqa: F401  (hipcc links libamdhip64: torch's runtime first, see capi.lib())
        L = C.CDLL(str(LIB))
        cfgp, gp, fp, ip = C.POINTER(Configuration), C.POINTER(GridDesc), C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.vpta_render.argtypes = [cfgp, gp, C.c_uint32, fp, fp]
        L.vpta_tau_at.argtypes = [cfgp, gp, fp, fp, C.c_uint64, fp]
        L.vptd_levels.argtypes = [C.c_uint32, fp, fp]
        L.vptd_render.argtypes = [cfgp, gp, C.c_uint32, C.c_uint32, fp, fp, fp]
        L.vptd_tau_upto.argtypes = [cfgp, gp, ip, ip, fp, C.c_uint64, fp]
        _L = L
    return _L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def render(cfg, density, sub=1, fill=0.0):
    """(alpha, tau) float32 [H][W] of the frame; `fill` is what the planes hold before the call."""
    alpha = np.full((cfg.height, cfg.width), fill, np.float32)
    tau = np.full((cfg.height, cfg.width), fill, np.float32)
    rc = lib().vpta_render(C.byref(cfg), C.byref(density.desc), int(sub), _fp(alpha), _fp(tau))
    assert rc == 0, rc
    return alpha, tau


def tau_at(cfg, density, rx, ry):
    """Optical depths float32 [n] of the camera rays through the raster points (rx[i], ry[i])."""
    rx, ry = np.ascontiguousarray(rx, np.float32).ravel(), np.ascontiguousarray(ry, np.float32).ravel()
    assert rx.shape == ry.shape
    tau = np.zeros(rx.size, np.float32)
    rc = lib().vpta_tau_at(C.byref(cfg), C.byref(density.desc), _fp(rx), _fp(ry), rx.size, _fp(tau))
    assert rc == 0, rc
    return tau
