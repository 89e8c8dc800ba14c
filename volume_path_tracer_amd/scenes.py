"""Scene configurations: the reference's scene files and the BASELINE.json workloads.

The reference's scenes (scenes/wdas_cloud.json, fire.json, fire_lowscattering.json) ship in
``volume_path_tracer_amd/scenes/`` and are read with the strict reader (vpt_config_read, mirroring
read_configuration, src/configuration.cpp:8-22).  Their volumes (volumes/*.nvdb) are not available,
so the BASELINE configs run on synthetic stand-ins:

  C1  wdas_cloud 256x256, 4 spp, CPU worker pool            -> cloud 512^3 stand-in
  C2  constant-density 128^3, 512x512, 64 spp               -> synth kind 0
  C3  wdas_cloud 1920x1080, 256 spp                         -> cloud 512^3 stand-in
  C4  fire 1920x1080, 256 spp                               -> cloud 512^3 + temperature 40*base
  C5  wdas_cloud 3840x2160, 1024 spp, 8 GPUs                -> cloud 512^3 stand-in

The stand-in camera looks at the synthetic volume (centred at the world origin) from (0, 0, -D):
D = 800 for the 512^3 volumes, 300 for the 128^3 one; every other parameter is the scene file's.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path

from . import capi

SCENE_DIR = Path(__file__).resolve().parent / "scenes"


def read_configuration(path) -> capi.Configuration:
    cfg = capi.Configuration()
    capi.check(capi.lib().vpt_config_read(str(path).encode(), C.byref(cfg)), f"read_configuration({path})")
    return cfg


def parse_configuration(text: str) -> capi.Configuration:
    cfg = capi.Configuration()
    b = text.encode()
    capi.check(capi.lib().vpt_config_parse(b, len(b), C.byref(cfg)), "parse_configuration")
    return cfg


def scene(name: str) -> capi.Configuration:
    return read_configuration(SCENE_DIR / f"{name}.json")


def orbit(cfg: capi.Configuration, frames: int, degrees: float = 360.0, closing: bool = False) -> list:
    """A turntable: `frames` configurations, frame k with the camera position rotated by degrees * k / frames about the
    axis through `look` along the normalised `up` (right-handed); look, up, vfov and everything else are cfg's.
    Frame 0 is cfg's camera bit for bit, and a full turn does not repeat it at the end (frame `frames` would).  The
    rotation is computed in float64 and rounded once to the configuration's floats.  closing: the rotation at index
    `frames` is appended (frames + 1 configurations): where the last frame's shutter closes (--shutter)."""
    import numpy as np

    frames = int(frames)
    if frames < 1:
        raise ValueError("orbit: at least one frame")
    cp = cfg.camera_parameters
    pos, look, up = (np.asarray(v[:], np.float64) for v in (cp.position, cp.look, cp.up))
    n = float(np.sqrt(up @ up))
    if not n > 0.0 or not np.isfinite(n):
        raise ValueError("orbit: the camera's up vector has no direction")
    axis, r = up / n, pos - look
    out = []
    for k in range(frames + 1 if closing else frames):
        c = cfg.copy()
        a = np.radians(float(degrees) * k / frames)
        if a != 0.0:  # Rodrigues' rotation of the offset from `look`
            p = look + r * np.cos(a) + np.cross(axis, r) * np.sin(a) + axis * (axis @ r) * (1.0 - np.cos(a))
            c.camera_parameters.position[:] = [float(v) for v in p.astype(np.float32)]
        out.append(c)
    return out


def light_gains(cfg_rendered: capi.Configuration, cfg_wanted: capi.Configuration):
    """The 3 x 3 relighting gains [group][XYZ] (float32; Integrator.relight, image.relight) that turn the light groups
    rendered under cfg_rendered into cfg_wanted's picture: row 0 (emission) the le_scale ratio, row 1 (sun) the ratio
    of distant_light.xyz * multiplier per channel, row 2 (sky) that of infinite_light.xyz * multiplier.  The products
    are the scene's float32 ones, the ratios float64 rounded once.  A source that is zero in both gets gain 1.
    ValueError where a rendered value is zero and the wanted one is not (nothing to scale), and when anything else
    differs that changes the paths or the emission non-linearly: camera, medium coefficients, g, max_depth,
    temperature scale or offset, sun direction, jitter, single-pixel mode, seed, waves, frame or tile size, volume."""
    import numpy as np

    a, b = cfg_rendered.copy(), cfg_wanted.copy()

    def sources(c):
        w, f = c.worker_parameters, np.float32
        return np.stack([np.full(3, c.volume_parameters.le_scale, np.float32),
                         np.asarray(w.distant_light_xyz[:], np.float32) * f(w.distant_light_multiplier),
                         np.asarray(w.infinite_light_xyz[:], np.float32) * f(w.infinite_light_multiplier)])

    have, want = sources(a), sources(b)
    for c in (a, b):  # what is left must be the same scene
        w = c.worker_parameters
        c.volume_parameters.le_scale = 0.0
        w.distant_light_multiplier = w.infinite_light_multiplier = 0.0
        w.distant_light_xyz[:] = w.infinite_light_xyz[:] = [0.0, 0.0, 0.0]
        c.num_workers = 0
    if bytes(a) != bytes(b):
        raise ValueError("light_gains: the configurations differ in more than the strength and colour of their lights "
                         "(camera, medium, g, max_depth, temperature mapping, sun direction, seed and sizes must agree)")
    names = ("le_scale", "distant_light", "infinite_light")
    k = np.ones((3, 3), np.float32)
    for g in range(3):
        for c in range(3):
            if have[g, c] == 0.0:
                if want[g, c] != 0.0:
                    raise ValueError(f"light_gains: {names[g]} channel {'XYZ'[c]} was rendered at zero: nothing to scale")
            else:
                k[g, c] = np.float32(np.float64(want[g, c]) / np.float64(have[g, c]))
    return k


_CAMERA_KEYS = {"position": 3, "look": 3, "up": 3, "vfov_deg": 1}


def read_camera_path(path) -> list:
    """A camera path: a JSON list of {"position": [x, y, z], "look": [x, y, z], "up"?: [x, y, z], "vfov_deg"?: v}, one
    per frame -> a list of dicts of floats (what Integrator.set_camera takes as keywords; an absent optional key keeps
    the scene's value).  Strict like read_configuration: an unknown key, a missing position or look, a wrong length
    or a non-number is a ValueError."""
    import json

    with open(path, "r", encoding="utf-8") as f:
        data = json.load(f)
    if not isinstance(data, list) or not data:
        raise ValueError(f"{path}: a camera path is a non-empty JSON list of cameras")
    return [_camera_entry(cam, f"{path}: frame {i}") for i, cam in enumerate(data)]


def _camera_entry(cam, where: str) -> dict:
    """One camera object of a camera path (or --shutter-camera's file), checked as read_camera_path states."""
    if not isinstance(cam, dict):
        raise ValueError(f"{where}: a camera is an object")
    for k in cam:
        if k not in _CAMERA_KEYS:
            raise ValueError(f"{where}: unknown key {k!r}")
    for k in ("position", "look"):
        if k not in cam:
            raise ValueError(f"{where}: missing key {k!r}")
    d = {}
    for k, v in cam.items():
        vals = v if _CAMERA_KEYS[k] == 3 else [v]
        if (not isinstance(vals, list) or len(vals) != _CAMERA_KEYS[k]
                or any(isinstance(x, bool) or not isinstance(x, (int, float)) for x in vals)):
            raise ValueError(f"{where}: {k!r} wants {_CAMERA_KEYS[k]} number(s)")
        d[k] = [float(x) for x in vals] if _CAMERA_KEYS[k] == 3 else float(v)
    return d


def read_camera(path) -> dict:
    """One camera: a JSON object in the keys and with the strictness of a read_camera_path entry (--shutter-camera)."""
    import json

    with open(path, "r", encoding="utf-8") as f:
        return _camera_entry(json.load(f), str(path))


def with_camera(cfg: capi.Configuration, position=None, look=None, up=None, vfov_deg=None) -> capi.Configuration:
    """A copy of cfg with the camera fields given replaced (a read_camera_path entry as keywords)."""
    c = cfg.copy()
    cp = c.camera_parameters
    for name, v in (("position", position), ("look", look), ("up", up)):
        if v is not None:
            getattr(cp, name)[:] = [float(x) for x in v]
    if vfov_deg is not None:
        cp.vfov_deg = float(vfov_deg)
    return c


def camera_of(cfg: capi.Configuration) -> dict:
    """cfg's camera as the dict with_camera and Integrator.set_camera take as keywords (floats as the configuration
    holds them)."""
    cp = cfg.camera_parameters
    return {"position": [float(v) for v in cp.position], "look": [float(v) for v in cp.look],
            "up": [float(v) for v in cp.up], "vfov_deg": float(cp.vfov_deg)}


def shutter_times(n: int) -> list:
    """The times in (0, 1) at which a shutter of n cameras samples the camera's move, in van der Corput order:
    t_k = radical_inverse_2(k) + 2^-(m + 1), 2^m the smallest power of two >= n.  Every prefix of 2^j times has one
    time in each interval of width 2^-j, so a tile that adaptive sampling stops after a few waves has still seen the
    whole shutter, not its first part.  Exact in float64 (dyadic rationals)."""
    n = int(n)
    if not 1 <= n <= capi.VPT_SHUTTER_MAX:
        raise ValueError(f"shutter_times: 1 .. {capi.VPT_SHUTTER_MAX} cameras")
    m = (n - 1).bit_length()
    out = []
    for k in range(n):
        r, f, i = 0.0, 0.5, k
        while i:
            if i & 1:
                r += f
            f *= 0.5
            i >>= 1
        out.append(r + 2.0 ** -(m + 1))
    return out


def lerp_camera(cam_open: dict, cam_close: dict, t: float) -> dict:
    """The camera at time t of the move from cam_open (t = 0) to cam_close (t = 1): every field a + (b - a) t in
    float64, rounded once to float32; t = 0 and t = 1 return the inputs' floats bit for bit.  Both are dicts of all
    four camera keys (camera_of)."""
    import numpy as np

    out = {}
    for k, n in _CAMERA_KEYS.items():
        if k not in cam_open or k not in cam_close:
            raise ValueError(f"lerp_camera: both cameras need {k!r} (camera_of(cfg) has every key)")
        a = np.asarray(cam_open[k], np.float64).reshape(n)
        b = np.asarray(cam_close[k], np.float64).reshape(n)
        v = a if t == 0.0 else b if t == 1.0 else a + (b - a) * float(t)
        v = [float(x) for x in v.astype(np.float32)]
        out[k] = v if n == 3 else v[0]
    return out


def shutter_cameras(cam_open: dict, cam_close: dict, n: int, times=None) -> list:
    """The n cameras of a shutter that opens on cam_open and closes on cam_close (Integrator.set_shutter's list):
    lerp_camera at shutter_times(n) (or at `times`)."""
    ts = shutter_times(n) if times is None else list(times)
    return [lerp_camera(cam_open, cam_close, t) for t in ts]


def shutter_entries(cfg: capi.Configuration, cameras):
    """cameras (dicts of set_camera's keywords; an absent key keeps cfg's value) as the ctypes array
    vpt_gpu_set_shutter takes."""
    cams = list(cameras)
    if not 1 <= len(cams) <= capi.VPT_SHUTTER_MAX:
        raise ValueError(f"a shutter holds 1 .. {capi.VPT_SHUTTER_MAX} cameras")
    arr = (capi.ShutterCamera * len(cams))()
    for e, cam in zip(arr, cams):
        for k in cam:
            if k not in _CAMERA_KEYS:
                raise ValueError(f"shutter camera: unknown key {k!r}")
        cp = with_camera(cfg, **cam).camera_parameters
        e.position[:], e.look[:], e.up[:], e.vfov_deg = cp.position[:], cp.look[:], cp.up[:], cp.vfov_deg
    return arr


def _standin_camera(cfg: capi.Configuration, distance: float) -> None:
    cp = cfg.camera_parameters
    cp.position[:] = [0.0, 0.0, -float(distance)]
    cp.look[:] = [0.0, 0.0, 0.0]
    cp.up[:] = [0.0, 1.0, 0.0]


@dataclass
class Workload:
    name: str
    cfg: capi.Configuration
    density_kind: int      # synthetic grid kind for the density (vpt_synth_grid)
    grid_n: int            # lattice size
    temperature: bool      # temperature grid (kind 2) present

    @property
    def spp(self) -> int:
        return int(self.cfg.num_waves)

    @property
    def samples(self) -> int:
        return self.cfg.width * self.cfg.height * self.spp


def workload(name: str, *, width=None, height=None, spp=None, grid_n=None) -> Workload:
    """BASELINE.json configs by short name: c1, c2, c3, c4, c5 (overrides for tests)."""
    name = name.lower()
    if name in ("c1", "c3", "c5"):
        cfg = scene("wdas_cloud")
        w, h, s = {"c1": (256, 256, 4), "c3": (1920, 1080, 256), "c5": (3840, 2160, 1024)}[name]
        kind, n, temp, dist = 1, 512, False, 800.0
    elif name == "c4":
        cfg = scene("fire")
        w, h, s = 1920, 1080, 256
        kind, n, temp, dist = 1, 512, True, 800.0
    elif name == "c2":
        # Homogeneous check: lights and max_depth from wdas_cloud.json, sigma_s 0.15, sigma_a 0,
        # g 0.4, le_scale 0.
        cfg = scene("wdas_cloud")
        v = cfg.volume_parameters
        v.sigma_s, v.sigma_a, v.henyey_greenstein_g, v.le_scale = 0.15, 0.0, 0.4, 0.0
        w, h, s = 512, 512, 64
        kind, n, temp, dist = 0, 128, False, 300.0
    else:
        raise KeyError(name)
    cfg.output_size[0] = int(width or w)
    cfg.output_size[1] = int(height or h)
    cfg.num_waves = int(spp or s)
    n = int(grid_n or n)
    _standin_camera(cfg, dist * n / (128 if kind == 0 else 512))
    return Workload(name, cfg, kind, n, temp)


class SynthGrid:
    """A synthetic grid generated by the product library (vpt_synth_grid), owning its arrays."""

    def __init__(self, kind: int, n: int):
        self.ptr = capi.lib().vpt_synth_grid(kind, n)
        if not self.ptr:
            raise RuntimeError(capi.lib().vpt_last_error().decode())
        self.desc = self.ptr.contents

    def grid(self, copy=True) -> capi.Grid:
        return capi.Grid.from_desc(self.desc, copy=copy)

    def __del__(self):
        try:
            capi.lib().vpt_synth_free(self.ptr)
        except Exception:
            pass
