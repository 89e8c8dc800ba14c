"""Camera motion blur on the CPU: the device state machine with a shutter Env (tests/native/shutter_host.cpp) against
the ordered sum of the oracle's per-wave films, each rendered with that wave's camera (tests/shutter_lib.py Reference),
bit for bit; scenes.shutter_times / shutter_cameras; the factored camera derivation against the oracle's camera matrix;
and the command line's refusals, which need no device."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import shutter_lib as SH
from volume_path_tracer_amd import capi, scenes
from volume_path_tracer_amd.scenes import SynthGrid, workload

# (workload, width, height, waves, cameras): ragged tiles and three unlike cameras; a full wavefront's worth of
# waves of one tile with 64 cameras, two of which wrap; a modulus that is no power of two
CASES = [("c3", 20, 12, 3, "three"), ("c4", 20, 12, 3, "three"), ("c3", 16, 8, 66, 64), ("c3", 16, 8, 66, 5)]
_cache = {}


def case(name, w, h, waves, cams):
    key = (name, w, h, waves, cams)
    if key not in _cache:
        wl = workload(name, width=w, height=h, spp=waves, grid_n=64)
        dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
        temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
        cameras = SH.three_cameras(wl.cfg) if cams == "three" else SH.moving_cameras(wl.cfg, cams)
        ref = SH.Reference(wl.cfg, dens, temp, cameras, waves)
        _cache[key] = (wl.cfg, dens, temp, cameras, ref)
    return _cache[key]


@pytest.mark.parametrize("name,w,h,waves,cams", CASES)
def test_host_film_is_the_ordered_sum_of_the_oracle_wave_films(name, w, h, waves, cams):
    cfg, dens, temp, cameras, ref = case(name, w, h, waves, cams)
    T = cfg.jobs_per_wave()
    film, rec, cnt = SH.host_render(cfg, dens, temp, cameras, 0, waves * T)
    assert cnt == ref.counters
    assert np.array_equal(np.nan_to_num(rec, nan=-1.0).view(np.uint32),
                          np.nan_to_num(ref.rec.reshape(-1, 3), nan=-1.0).view(np.uint32))
    assert SH.same_bits(film, ref.film())
    assert (film[..., 3] == waves).all()
    # the cameras matter: the still frame is another film
    still, _, _ = O.render_jobs(cfg, O.OracleGrid(dens, fix_majorants=True),
                                O.OracleGrid(temp, fix_majorants=False) if temp is not None else None, 0, waves * T)
    assert not SH.same_bits(film, still)


def test_host_jobs_from_a_later_wave_take_that_waves_camera():
    """A job range that starts at wave 1: the entry is (jid / T) % n of the job id, not of the launch's index."""
    cfg, dens, temp, cameras, ref = case(*CASES[0])
    T = cfg.jobs_per_wave()
    film, rec, _ = SH.host_render(cfg, dens, temp, cameras, T, 2 * T)
    assert np.array_equal(np.nan_to_num(rec, nan=-1.0).view(np.uint32),
                          np.nan_to_num(ref.rec[1:].reshape(-1, 3), nan=-1.0).view(np.uint32))


def test_shutter_times():
    for n in (1, 2, 3, 5, 64, 100, 256):
        t = scenes.shutter_times(n)
        assert len(t) == n and all(0.0 < x < 1.0 for x in t) and len(set(t)) == n
        j = 0
        while (1 << j) <= n:
            cells = sorted(int(x * (1 << j)) for x in t[:1 << j])
            assert cells == list(range(1 << j)), (n, j)
            j += 1
    assert scenes.shutter_times(4) == [0.125, 0.625, 0.375, 0.875]
    for bad in (0, 65537):
        with pytest.raises(ValueError):
            scenes.shutter_times(bad)


def test_shutter_cameras_endpoints_and_rounding():
    a = {"position": [0.1, -0.0, 3.0], "look": [1e-3, 2.5, -7.0], "up": [0.0, 1.0, 0.0], "vfov_deg": 33.3}
    a = {k: ([float(np.float32(x)) for x in v] if isinstance(v, list) else float(np.float32(v))) for k, v in a.items()}
    b = {"position": [9.7, 4.0, -3.0], "look": [0.3, 2.0, -6.0], "up": [0.1, 0.9, 0.0], "vfov_deg": 50.0}
    b = {k: ([float(np.float32(x)) for x in v] if isinstance(v, list) else float(np.float32(v))) for k, v in b.items()}
    ends = scenes.shutter_cameras(a, b, 2, times=[0.0, 1.0])

    def bits(cam):
        return np.concatenate([np.asarray(cam[k], np.float32).reshape(-1) for k in ("position", "look", "up", "vfov_deg")]
                              ).view(np.uint32)

    assert np.array_equal(bits(ends[0]), bits(a)) and np.array_equal(bits(ends[1]), bits(b))  # (the -0.0 included)
    cams = scenes.shutter_cameras(a, b, 5)
    for cam, t in zip(cams, scenes.shutter_times(5)):
        want = np.float32(np.float64(a["vfov_deg"]) + (np.float64(b["vfov_deg"]) - np.float64(a["vfov_deg"])) * t)
        assert np.float32(cam["vfov_deg"]) == want
        wp = (np.asarray(a["position"], np.float64) + (np.asarray(b["position"], np.float64)
                                                       - np.asarray(a["position"], np.float64)) * t).astype(np.float32)
        assert np.array_equal(np.asarray(cam["position"], np.float32), wp)
    with pytest.raises(ValueError):
        scenes.lerp_camera({"position": [0, 0, 0]}, b, 0.5)


def test_factored_camera_derivation_is_the_oracle_camera_matrix():
    cfg = workload("c3", width=20, height=12, spp=1, grid_n=64).cfg
    cams = SH.three_cameras(cfg) + SH.moving_cameras(cfg, 5) + [{}]
    arr = scenes.shutter_entries(cfg, cams)
    fp = C.POINTER(C.c_float)
    for e, cam in zip(arr, cams):
        out = np.full(16, np.nan, np.float32)
        assert capi.lib().vpt_shutter_entry(C.byref(e), cfg.width, cfg.height, out.ctypes.data_as(fp)) == 0
        c = scenes.with_camera(cfg, **cam)
        L, t = np.zeros(9, np.float32), np.zeros(3, np.float32)
        O.lib().vpto_camera_matrix(C.byref(c), L.ctypes.data_as(fp), t.ctypes.data_as(fp))
        rows = out[:12].reshape(3, 4)
        assert SH.same_bits(rows[:, :3].reshape(-1), L) and SH.same_bits(rows[:, 3], t)
        assert SH.same_bits(out[12:15], np.asarray(c.camera_parameters.position[:], np.float32)) and out[15] == 0
    bad = scenes.shutter_entries(cfg, [{"look": list(cfg.camera_parameters.position)}])
    out = np.zeros(16, np.float32)
    assert capi.lib().vpt_shutter_entry(C.byref(bad[0]), cfg.width, cfg.height, out.ctypes.data_as(fp)) == 1  # VPT_E_INVALID


REFUSED = [("--alpha", ["--alpha"]), ("--alpha-foreground", ["--alpha-foreground"]), ("--denoise", ["--denoise"]),
           ("--adaptive-fused", ["--adaptive", "0.05", "--adaptive-fused"]), ("--rng-mode pixel", ["--rng-mode", "pixel"]),
           ("--event-log", ["--event-log", "ev.csv"])]


@pytest.mark.parametrize("named,extra", REFUSED, ids=[r[0] for r in REFUSED])
def test_cli_refuses_what_a_shutter_cannot_honour(tmp_path, named, extra):
    """Exit 1 naming the option, before a device is touched: no device is visible to the child."""
    cam = tmp_path / "close.json"
    cam.write_text(json.dumps({"position": [5.0, 0.0, -100.0], "look": [0.0, 0.0, 0.0]}))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    extra = [str(tmp_path / a) if a.endswith(".csv") else a for a in extra]
    r = subprocess.run([sys.executable, "-m", "volume_path_tracer_amd", str(scenes.SCENE_DIR / "wdas_cloud.json"),
                        str(tmp_path / "o.png"), "--synthetic", "cloud:64", "--size", "16x8", "--spp", "2",
                        "--shutter-camera", str(cam), *extra], capture_output=True, text=True, env=env, cwd=str(SH.ROOT))
    assert r.returncode == 1, (r.returncode, r.stderr[-2000:])
    assert named in r.stderr and "shutter" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "o.png").exists()


def test_cli_shutter_argument_rules(tmp_path):
    """--shutter needs a sequence with a moving camera, --shutter-camera a single frame; both exit 1 from the arguments."""
    cam = tmp_path / "close.json"
    cam.write_text(json.dumps({"position": [5.0, 0.0, -100.0], "look": [0.0, 0.0, 0.0]}))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    base = [sys.executable, "-m", "volume_path_tracer_amd", str(scenes.SCENE_DIR / "wdas_cloud.json")]
    for extra in (["--shutter", "0.5"], ["--frames", "2", "--shutter", "1.5"], ["--frames", "2", "--shutter-camera", str(cam)],
                  ["--shutter-camera", str(cam), "--shutter-samples", "0"]):
        out = str(tmp_path / ("o_%d.png" if "--frames" in extra else "o.png"))
        r = subprocess.run([*base, out, "--synthetic", "cloud:64", "--size", "16x8", "--spp", "2", *extra],
                           capture_output=True, text=True, env=env, cwd=str(SH.ROOT))
        assert r.returncode == 1 and "shutter" in r.stderr, (extra, r.returncode, r.stderr[-1000:])
