"""Camera motion blur (vpt_gpu_set_shutter), shared by tests/test_shutter_host.py and tests/test_gpu_shutter.py:

* the reference.  The oracle (tests/oracle_lib.py) is not changed: a job's RNG stream depends on its jid alone and the
  ordered film adds a pixel's samples in wave order, so the shuttered film is the ordered fp32 sum of the films the
  oracle renders wave by wave, wave k with the scene whose camera is entry k % n.  Each per-wave film holds one sample
  per pixel (0 + 1 and 0 + r * L, both exact), so adding the per-wave films in wave order is exactly the ordered film's
  arithmetic;
* the same sum through light_groups_lib.isolated_oracle for the light-group planes, and the per-sample records for
  the moment plane (adaptive_ref.accumulate);
* the ctypes binding of tests/native/shutter_host.cpp (the device state machine on the CPU with a shutter Env), compiled
  host-only with hipcc as tests/light_groups_lib.py compiles its library.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

import adaptive_ref as AR
import oracle_lib as O
from volume_path_tracer_amd import scenes
from volume_path_tracer_amd.capi import Configuration, Counters, GridDesc, ShutterCamera

ROOT = Path(__file__).resolve().parents[1]
NATIVE = ROOT / "tests" / "native"
CSRC = ROOT / "volume_path_tracer_amd" / "csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = [NATIVE / "shutter_host.cpp", CSRC / "vpt_scene.cpp", CSRC / "vpt_grid_build.cpp", CSRC / "vpt_config.cpp"]
# hostsim's flags (tests/native/Makefile): no contraction, the device's semantics on the host
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "--cuda-host-only",
         "-shared"]
LIB = NATIVE / "build" / "libvpt_shutter_host.so"
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
        L.vptsh_render_jobs.argtypes = [cfgp, gp, gp, C.POINTER(ShutterCamera), C.c_uint32, C.c_uint64, C.c_uint64, fp, fp,
                                        C.POINTER(Counters)]
        _L = L
    return _L


def host_render(cfg, density, temperature, cameras, jid_begin, jid_count):
    """The host state machine with a shutter Env -> (film [H][W][4], records [jid_count * area][3], counters)."""
    area = int(cfg.tile_size[0] * cfg.tile_size[1])
    film = np.zeros((cfg.height, cfg.width, 4), np.float32)
    rec = np.full((jid_count * area, 3), np.nan, np.float32)
    cnt = Counters()
    arr = scenes.shutter_entries(cfg, cameras)
    fp = C.POINTER(C.c_float)
    rc = lib().vptsh_render_jobs(C.byref(cfg), C.byref(density.desc),
                                 C.byref(temperature.desc) if temperature is not None else None, arr, len(arr), jid_begin,
                                 jid_count, film.ctypes.data_as(fp), rec.ctypes.data_as(fp), C.byref(cnt))
    assert rc == 0, rc
    return film, rec, cnt.as_dict()


# ---- the cameras of the cases ----------------------------------------------------------------------------------------

def three_cameras(cfg):
    """Three distinct cameras: the position moved, the look moved, the field of view changed (the rest the scene's)."""
    cp = cfg.camera_parameters
    p, l = [float(v) for v in cp.position], [float(v) for v in cp.look]
    return [{"position": [p[0] + 7.0, p[1] - 3.0, p[2] + 5.0]},
            {"look": [l[0] - 4.0, l[1] + 6.0, l[2] + 1.0]},
            {"vfov_deg": float(cp.vfov_deg) * 0.75}]


def moving_cameras(cfg, n):
    """n distinct cameras of a move (scenes.shutter_cameras: van der Corput times between an open and a close camera)."""
    a = scenes.camera_of(cfg)
    b = dict(a, position=[a["position"][0] + 30.0, a["position"][1] + 12.0, a["position"][2] - 9.0],
             look=[a["look"][0] + 5.0, a["look"][1] - 2.0, a["look"][2]], vfov_deg=a["vfov_deg"] * 1.1)
    return scenes.shutter_cameras(a, b, n)


# ---- the reference ---------------------------------------------------------------------------------------------------

class Reference:
    """The oracle's per-wave runs of waves [wave_begin, wave_begin + waves) with wave k's camera cameras[k % n]:
    rec [waves][T * area][3] (per-sample L), wave_films [waves][H][W][4], counters (summed); with groups=True also
    group_wave_films [waves][3][H][W][4] from light_groups_lib.isolated_oracle."""

    def __init__(self, cfg, dens, temp, cameras, waves, wave_begin=0, groups=False):
        self.cfg, self.waves, self.wave_begin = cfg, waves, wave_begin
        T = cfg.jobs_per_wave()
        od = O.OracleGrid(dens, fix_majorants=True)
        ot = O.OracleGrid(temp, fix_majorants=False) if temp is not None else None
        self.wave_films, self.rec, self.group_wave_films = [], [], []
        self.counters = None
        for k in range(wave_begin, wave_begin + waves):
            c = scenes.with_camera(cfg, **cameras[k % len(cameras)])
            if groups:
                import light_groups_lib as LG

                iso = LG.isolated_oracle(c, dens, temp, k * T, T)
                film, rec, cnt = iso["film"], iso["rec"], iso["counters"]
                self.group_wave_films.append(iso["group_films"])
            else:
                film, rec, cnt = O.render_jobs(c, od, ot, k * T, T, records=True)
            assert np.isin(film[..., 3], (0.0, 1.0)).all()  # (one sample per pixel: the wave's film is 0 + its adds)
            self.wave_films.append(film)
            self.rec.append(rec)
            self.counters = cnt if self.counters is None else {n: self.counters[n] + cnt[n] for n in cnt}
        self.rec = np.stack(self.rec)

    def film(self, waves=None, tiles=None, fill=0.0):
        """sum_k film_k in wave order, fp32, over the first `waves` waves; tiles: only those tiles' pixels (the others
        keep `fill`)."""
        waves = self.waves if waves is None else waves
        out = np.zeros_like(self.wave_films[0])
        for k in range(waves):
            out = out + self.wave_films[k]
        return self._only(out, tiles, fill)

    def group_films(self, tiles=None, fill=0.0):
        out = np.zeros_like(self.group_wave_films[0])
        for k in range(self.waves):
            out = out + self.group_wave_films[k]
        return np.stack([self._only(out[g], tiles, fill) for g in range(3)])

    def states(self):
        """adaptive_ref.accumulate over the records: (films, m2s) after every wave, waves + 1 states each."""
        return AR.accumulate(self.cfg, AR.records_to_samples(self.cfg, self.rec.reshape(-1, 3), 0, self.waves))

    def _only(self, film, tiles, fill):
        if tiles is None:
            return film
        m = AR.tile_mask(self.cfg, tiles)
        out = np.full_like(film, fill)
        out[m] = film[m]
        return out


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
