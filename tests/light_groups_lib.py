"""Light groups (vpt_gpu_set_light_groups), shared by tests/test_light_groups_host.py and tests/test_gpu_light_groups.py:

* the oracle's isolated films.  The oracle (tests/oracle_lib.py) is not changed: its draw sequence does not depend on
  the strength of a light (apart from sample_Ld's test Li == 0), so a run with the other sources switched off renders
  one group alone.  isolated_oracle() does those runs and asserts, for every case it is given, that each run had the
  plain run's counters (all eleven fields), that every value is finite, and that the two ways to a plane agree;
* the ctypes binding of tests/native/light_groups_host.cpp (the device state machine on the CPU with a groups Env),
  compiled host-only with hipcc like tests/eval_split_lib.py compiles its library;
* the film passes restated in numpy over per-sample records, plain and band layout.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

import oracle_lib as O
from volume_path_tracer_amd.capi import Configuration, Counters, GridDesc

ROOT = Path(__file__).resolve().parents[1]
NATIVE = ROOT / "tests" / "native"
CSRC = ROOT / "volume_path_tracer_amd" / "csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = [NATIVE / "light_groups_host.cpp", CSRC / "vpt_scene.cpp", CSRC / "vpt_grid_build.cpp", CSRC / "vpt_config.cpp"]
# hostsim's flags (tests/native/Makefile): no contraction, the device's semantics on the host
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "--cuda-host-only",
         "-shared"]
LIB = NATIVE / "build" / "libvpt_light_groups_host.so"
_L = None
GROUPS = ("emission", "sun", "sky")


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
        L.vptlg_render_waves.argtypes = [cfgp, gp, gp, C.c_uint64, C.c_uint32, C.c_uint32, fp, fp, fp, C.POINTER(Counters)]
        L.vptlg_band_floats.argtypes = [C.c_uint32] * 4
        L.vptlg_band_floats.restype = C.c_uint64
        L.vptlg_band_slot.argtypes = [C.c_uint32] * 6
        L.vptlg_band_slot.restype = C.c_uint64
        _L = L
    return _L


def host_render_waves(cfg, density, temperature, wave_begin, waves, G):
    """The host state machine with a groups Env over `waves` whole waves -> (beauty film, plain [4][jobs * area][3],
    band [4][band floats], counters): regions beauty, emission, sun, sky in both layouts."""
    T, area = cfg.jobs_per_wave(), int(cfg.tile_size[0] * cfg.tile_size[1])
    film = np.zeros((cfg.height, cfg.width, 4), np.float32)
    plain = np.full((4, waves * T * area, 3), np.nan, np.float32)
    band = np.full((4, int(lib().vptlg_band_floats(T, waves, area, G))), np.nan, np.float32)
    cnt = Counters()
    fp = C.POINTER(C.c_float)
    rc = lib().vptlg_render_waves(C.byref(cfg), C.byref(density.desc),
                                  C.byref(temperature.desc) if temperature is not None else None, wave_begin, waves, G,
                                  film.ctypes.data_as(fp), plain.ctypes.data_as(fp), band.ctypes.data_as(fp), C.byref(cnt))
    assert rc == 0, rc
    return film, plain, band, cnt.as_dict()


# ---- the oracle's isolated films -------------------------------------------------------------------------------------

def _variant(cfg, le_scale=None, sky=None, sun_axis=None):
    c = cfg.copy()
    w = c.worker_parameters
    if le_scale is not None:
        c.volume_parameters.le_scale = le_scale
    if sky is not None:
        w.infinite_light_multiplier = sky
    if sun_axis is not None and _sun_on(cfg):  # (a sun that is off stays off: sample_Ld's Li == 0 changes the draws)
        w.distant_light_xyz[:] = [1.0 if k == sun_axis else 0.0 for k in range(3)]
        w.distant_light_multiplier = 1.0
    return c


def _sun_on(cfg) -> bool:
    w = cfg.worker_parameters
    li = np.asarray(w.distant_light_xyz[:], np.float32) * np.float32(w.distant_light_multiplier)
    return bool((li != 0).any())


def same_but_zero_sign(a, b):
    """a and b agree byte for byte after + 0.0f on both sides (a zero may carry either sign)."""
    a = np.asarray(a, np.float32) + np.float32(0)
    b = np.asarray(b, np.float32) + np.float32(0)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def isolated_oracle(cfg, dens, temp, jid_begin, jid_count):
    """-> dict: 'film' / 'rec' / 'counters' of the plain run and 'group_films' [3][H][W][4], 'group_recs' [3][N][3] of
    the isolated runs (emission, sun, sky), with the three conditions asserted:

    * sun: le_scale = 0, infinite_light.multiplier = 0;
    * emission, channel c: infinite_light.multiplier = 0 and distant_light.xyz the unit vector on another channel
      (shadow rays still traced; the sun adds + 0 to channel c): the unit X run gives Y and Z, the unit Y run X and Z;
    * sky, channel c: the same two runs with le_scale = 0 and the sky left on."""
    od = O.OracleGrid(dens, fix_majorants=True)
    ot = O.OracleGrid(temp, fix_majorants=False) if temp is not None else None

    def run(c):
        film, rec, cnt = O.render_jobs(c, od, ot, jid_begin, jid_count, records=True)
        return film, rec, cnt

    film, rec, counters = run(cfg)
    wp = cfg.worker_parameters
    runs = {
        "sun": run(_variant(cfg, le_scale=0.0, sky=0.0)),
        "em_x": run(_variant(cfg, sky=0.0, sun_axis=0)),
        "em_y": run(_variant(cfg, sky=0.0, sun_axis=1)),
        "sky_x": run(_variant(cfg, le_scale=0.0, sky=float(wp.infinite_light_multiplier), sun_axis=0)),
        "sky_y": run(_variant(cfg, le_scale=0.0, sky=float(wp.infinite_light_multiplier), sun_axis=1)),
    }
    for name, (f, r, cnt) in runs.items():
        assert cnt == counters, f"{name}: the isolating run's counters differ from the plain run's: a wrong choice of case"
        # (records of a ragged tile's missing pixels keep their NaN fill; a NaN sample would show in the film)
        assert np.isfinite(f).all() and np.array_equal(np.isfinite(r), np.isfinite(rec)), \
            f"{name}: a value is not finite: a wrong choice of case"
    assert np.isfinite(film).all()

    def channels(a, b, what):
        """X from the unit Y run b, Y from the unit X run a, Z from either (asserted identical); w likewise."""
        if _sun_on(cfg):
            out = []
            for fa, fb in ((a[0], b[0]), (a[1], b[1])):
                assert same_but_zero_sign(fa[..., 2], fb[..., 2]), f"{what}: the two channel choices give different planes"
                o = fa.copy()
                o[..., 0] = fb[..., 0]
                out.append(o)
            return out
        assert same_but_zero_sign(a[0], b[0]) and same_but_zero_sign(a[1], b[1]), what
        return [a[0], a[1]]

    em_f, em_r = channels(runs["em_x"], runs["em_y"], "emission")
    sky_f, sky_r = channels(runs["sky_x"], runs["sky_y"], "sky")
    return {"film": film, "rec": rec, "counters": counters,
            "group_films": np.stack([em_f, runs["sun"][0], sky_f]),
            "group_recs": np.stack([em_r, runs["sun"][1], sky_r])}


# ---- the film passes, restated ---------------------------------------------------------------------------------------

def _tile_pixels(cfg, t):
    """(q, px, py) of tile t's pixels inside the image, local index order."""
    tw, th = int(cfg.tile_size[0]), int(cfg.tile_size[1])
    ntx = -(-cfg.width // tw)
    x0, y0 = (t % ntx) * tw, (t // ntx) * th
    rw, rh = min(cfg.width - x0, tw), min(cfg.height - y0, th)
    q = np.arange(rw * rh)
    return q, x0 + q % rw, y0 + q // rw


def film_pass_plain(cfg, rec, waves, film=None):
    """vpt_film_order_kernel restated: rec [waves * T * area][3] (job w * T + t, local pixel q) added pixel by pixel in
    wave order: w = w + 1, xyz = xyz + imaging_ratio * L, float32."""
    T, area = cfg.jobs_per_wave(), int(cfg.tile_size[0] * cfg.tile_size[1])
    r = np.float32(cfg.camera_parameters.imaging_ratio)
    film = np.zeros((cfg.height, cfg.width, 4), np.float32) if film is None else film
    rec = rec.reshape(waves, T, area, 3)
    for t in range(T):
        q, px, py = _tile_pixels(cfg, t)
        for w in range(waves):
            film[py, px, 3] = film[py, px, 3] + np.float32(1)
            film[py, px, :3] = film[py, px, :3] + r * rec[w, t, q]
    return film


def film_pass_band(cfg, band, waves, G, film=None):
    """vpt_band_order_kernel restated over the lane-adjacent layout (band_slot): sample (tile tb, wave w, pixel q) at
    float ((((tb * groups + w // G) * area + q) * G) + w % G) * 3."""
    T, area = cfg.jobs_per_wave(), int(cfg.tile_size[0] * cfg.tile_size[1])
    groups = -(-waves // G)
    r = np.float32(cfg.camera_parameters.imaging_ratio)
    film = np.zeros((cfg.height, cfg.width, 4), np.float32) if film is None else film
    assert int(lib().vptlg_band_slot(1, G + 1 if waves > G else 0, 3, groups, area, G)) == \
        ((((1 * groups + (1 if waves > G else 0)) * area + 3) * G) + (1 if waves > G else 0)) * 3
    for t in range(T):
        q, px, py = _tile_pixels(cfg, t)
        for w in range(waves):
            at = ((((t * groups + w // G) * area + q) * G) + w % G) * 3
            L = np.stack([band[at], band[at + 1], band[at + 2]], axis=-1)
            film[py, px, 3] = film[py, px, 3] + np.float32(1)
            film[py, px, :3] = film[py, px, :3] + r * L
    return film
