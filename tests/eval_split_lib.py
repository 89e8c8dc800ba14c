"""ctypes binding of tests/native/eval_split_host.cpp: the device state machine on the CPU in two environments, the
density evaluation whole or split (Env::kEvalSplit).  The library is compiled with hipcc, host only, like
tests/alpha_lib.py compiles matte_host.cpp (tests/native/Makefile does not know it): on first use, or ahead of the
tests by __graft_entry__.build()."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

from volume_path_tracer_amd.capi import Configuration, Counters, GridDesc

ROOT = Path(__file__).resolve().parents[1]
NATIVE = ROOT / "tests" / "native"
CSRC = ROOT / "volume_path_tracer_amd" / "csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = [NATIVE / "eval_split_host.cpp", CSRC / "vpt_scene.cpp", CSRC / "vpt_grid_build.cpp", CSRC / "vpt_config.cpp"]
# hostsim's flags (tests/native/Makefile): no contraction, the device's semantics on the host
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "--cuda-host-only",
         "-shared"]
LIB = NATIVE / "build" / "libvpt_eval_split_host.so"
_L = None


def build_lib() -> Path:
    """The shared library, rebuilt when a source or header is newer."""
    deps = SOURCES + [NATIVE / "hostsim.cpp"] + sorted(CSRC.glob("*.h")) + [ROOT / "include" / "vpt_gpu.h"]
    if not LIB.exists() or LIB.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        LIB.parent.mkdir(parents=True, exist_ok=True)
        tmp = LIB.with_name(f"{LIB.name}.{os.getpid()}.tmp")
        r = subprocess.run([HIPCC, *FLAGS, "-o", str(tmp), *map(str, SOURCES)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        os.replace(tmp, LIB)
    return LIB


def lib():
    global _L
    if _L is None:
        build_lib()
        import torch  # noqa: F401  (hipcc links libamdhip64: torch's runtime first, see capi.lib())
        L = C.CDLL(str(LIB))
        cfgp, gp, fp = C.POINTER(Configuration), C.POINTER(GridDesc), C.POINTER(C.c_float)
        L.vptes_render_jobs.argtypes = [cfgp, gp, gp, C.c_uint64, C.c_uint64, fp, fp, C.POINTER(Counters), C.c_int,
                                        C.c_int, C.POINTER(C.c_uint64)]
        _L = L
    return _L


def render_jobs(cfg, density, temperature, jid_begin, jid_count, split, runs=-1):
    """(film, per-sample records, counters, the lane's final RNG state) of the jobs in jid order, every gate at 1."""
    film = np.zeros((cfg.height, cfg.width, 4), np.float32)
    tile_area = int(cfg.tile_size[0] * cfg.tile_size[1])
    rec = np.full((jid_count * tile_area, 3), np.nan, np.float32)
    cnt, rng = Counters(), C.c_uint64()
    fp = C.POINTER(C.c_float)
    rc = lib().vptes_render_jobs(C.byref(cfg), C.byref(density.desc),
                                 C.byref(temperature.desc) if temperature is not None else None, jid_begin, jid_count,
                                 film.ctypes.data_as(fp), rec.ctypes.data_as(fp), C.byref(cnt), int(bool(split)),
                                 int(runs), C.byref(rng))
    assert rc == 0, rc
    return film, rec, cnt.as_dict(), int(rng.value)
