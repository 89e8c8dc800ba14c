"""ctypes binding of tests/native/denoise_host.cpp: the denoiser's per-pixel functions (csrc/vpt_denoise.h, the code
the vpt_denoise kernels run per lane) over a frame on the CPU.  The library is compiled with hipcc, host only, like
alpha_lib.py compiles matte_host.cpp (tests/native/Makefile does not know it): on first use, or ahead of the tests by
__graft_entry__.build()."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

from volume_path_tracer_amd.capi import DenoiseParams

ROOT = Path(__file__).resolve().parents[1]
NATIVE = ROOT / "tests" / "native"
CSRC = ROOT / "volume_path_tracer_amd" / "csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = [NATIVE / "denoise_host.cpp"]
# hostsim's float flags (tests/native/Makefile): no contraction, the device's semantics on the host
FLAGS = ["-std=c++20", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "--cuda-host-only",
         "-I" + str(ROOT / "include")]
LIB = NATIVE / "build" / "libvpt_denoise_host.so"
_L = None


def compile_host(out: Path, extra=()) -> Path:
    """hipcc, host only: the library (extra = ["-O2", "-shared"]) or the stand-alone program (-DDENOISE_HOST_MAIN)."""
    out.parent.mkdir(parents=True, exist_ok=True)
    r = subprocess.run([HIPCC, *FLAGS, *extra, "-o", str(out), *map(str, SOURCES)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def build_lib() -> Path:
    """The shared library, rebuilt when its source or a header is newer (__graft_entry__.build() calls this too, so
    the tests of a built tree compile nothing)."""
    deps = SOURCES + [CSRC / "vpt_denoise.h", ROOT / "include" / "vpt_gpu.h"]
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
        fp = C.POINTER(C.c_float)
        L.vptd_denoise.argtypes = [C.c_int32, C.c_int32, C.POINTER(DenoiseParams), fp, fp, C.POINTER(fp), fp, fp]
        _L = L
    return _L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def denoise(film, m2, guides=(), guide_sigma=None, iterations=4, sigma_l=4.0, rel_floor=1e-3, fill=np.nan):
    """(out film float32[H][W][4], var float32[H][W]) of the host build; the outputs hold `fill` before the call."""
    film = np.ascontiguousarray(film, np.float32)
    m2 = np.ascontiguousarray(m2, np.float32)
    H, W = m2.shape
    assert film.shape == (H, W, 4)
    guides = [np.ascontiguousarray(g, np.float32) for g in guides]
    assert all(g.shape == (H, W) for g in guides)
    p = DenoiseParams.make(iterations, len(guides), sigma_l, rel_floor, guide_sigma)
    gp = (C.POINTER(C.c_float) * max(1, len(guides)))(*[_fp(g) for g in guides])
    out = np.full((H, W, 4), fill, np.float32)
    var = np.full((H, W), fill, np.float32)
    rc = lib().vptd_denoise(W, H, C.byref(p), _fp(film), _fp(m2), gp, _fp(out), _fp(var))
    assert rc == 0, rc
    return out, var
