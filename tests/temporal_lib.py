"""ctypes binding of tests/native/temporal_host.cpp: the temporal pass's per-pixel function (csrc/vpt_temporal.h, the
code vpt_temporal_kernel runs per lane) over a frame on the CPU.  The library is compiled with hipcc, host only, like
denoise_lib.py compiles denoise_host.cpp (tests/native/Makefile does not know it): on first use, or ahead of the tests
by __graft_entry__.build()."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

from volume_path_tracer_amd.capi import TemporalParams

ROOT = Path(__file__).resolve().parents[1]
NATIVE = ROOT / "tests" / "native"
CSRC = ROOT / "volume_path_tracer_amd" / "csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = [NATIVE / "temporal_host.cpp"]
# hostsim's float flags (tests/native/Makefile): no contraction, the device's semantics on the host
FLAGS = ["-std=c++20", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "--cuda-host-only",
         "-I" + str(ROOT / "include")]
LIB = NATIVE / "build" / "libvpt_temporal_host.so"
_L = None


def compile_host(out: Path, extra=()) -> Path:
    """hipcc, host only: the library (extra = ["-O2", "-shared"]) or the stand-alone program (-DTEMPORAL_HOST_MAIN)."""
    out.parent.mkdir(parents=True, exist_ok=True)
    r = subprocess.run([HIPCC, *FLAGS, *extra, "-o", str(out), *map(str, SOURCES)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def build_lib() -> Path:
    """The shared library, rebuilt when its source or a header is newer (__graft_entry__.build() calls this too, so
    the tests of a built tree compile nothing)."""
    deps = SOURCES + [CSRC / "vpt_temporal.h", ROOT / "include" / "vpt_gpu.h"]
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
        L.vptt_temporal.argtypes = [C.c_int32, C.c_int32, C.POINTER(TemporalParams), fp, fp, fp, fp, fp, fp, fp, fp, fp, fp,
                                    fp, fp]
        L.vptt_constants.argtypes = [fp, fp]
        _L = L
    return _L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def constants(prev16):
    """temporal_prev_constants of the host build: dict of n, a, b (3 floats each), tn, ta, tb."""
    prev16 = np.ascontiguousarray(prev16, np.float32)
    out = np.zeros(12, np.float32)
    assert lib().vptt_constants(_fp(prev16), _fp(out)) == 0
    return dict(n=out[0:3], a=out[3:6], b=out[6:9], tn=out[9], ta=out[10], tb=out[11])


def temporal(film, m2, depth, cur16, prev16, history=None, max_history=64.0, depth_tol=0.1, sigma_r=4.0, rel_floor=1e-3,
             fill=np.nan):
    """(out film [H][W][4], out m2 [H][W], motion [H][W][2], hist_n [H][W]) of the host build; the outputs hold `fill`
    before the call.  The signature of temporal_ref.temporal."""
    film = np.ascontiguousarray(film, np.float32)
    m2 = np.ascontiguousarray(m2, np.float32)
    depth = np.ascontiguousarray(depth, np.float32)
    cur16, prev16 = np.ascontiguousarray(cur16, np.float32), np.ascontiguousarray(prev16, np.float32)
    H, W = m2.shape
    assert film.shape == (H, W, 4) and depth.shape[1:] == (H, W) and cur16.shape == prev16.shape == (16,)
    hist = [None, None, None]
    if history is not None:
        hist = [np.ascontiguousarray(a, np.float32) for a in history]
        assert hist[0].shape == film.shape and hist[1].shape == m2.shape and hist[2].shape == depth.shape
    p = TemporalParams.make(depth.shape[0], max_history, depth_tol, sigma_r, rel_floor)
    out = np.full((H, W, 4), fill, np.float32)
    om2 = np.full((H, W), fill, np.float32)
    mv = np.full((H, W, 2), fill, np.float32)
    hn = np.full((H, W), fill, np.float32)
    rc = lib().vptt_temporal(W, H, C.byref(p), _fp(cur16), _fp(prev16), _fp(film), _fp(m2), _fp(depth), _fp(hist[0]),
                             _fp(hist[1]), _fp(hist[2]), _fp(out), _fp(om2), _fp(mv), _fp(hn))
    assert rc == 0, rc
    return out, om2, mv, hn
