"""Host driver: the reference's work-distribution API over the HIP integrator.

``TileProvider`` restates include/vpt/tile_provider.hpp / src/tile_provider.cpp (job id -> (tile,
wave), wave bookkeeping, stop_at_next_wave, progress/ETA).  ``run`` is the drop-in for
``vpt::run`` (src/worker.cpp:92-208): instead of tracing one token at a time on a CPU thread, it
drains the provider in contiguous job-id batches and launches each batch on the GPU.  Job ids key
the RNG streams (hash(seed, jid)), so the batching does not change any sample.

Device memory (film, per-sample records) is plain torch CUDA tensors — torch is plumbing here; the
integrator itself is the HIP kernel in libvpt_amd.so.
"""
from __future__ import annotations

import ctypes as C
import threading
import time
from typing import Optional

import numpy as np

from . import capi


def ceildiv(a: int, b: int) -> int:
    return a // b + (a % b != 0)


class TileProvider:
    """tile_provider.cpp:14-111 — job index -> (tile, wave); waves start when first touched."""

    def __init__(self, img_size, waves: int, tile_size):
        self.img_w, self.img_h = int(img_size[0]), int(img_size[1])
        self.tile_w, self.tile_h = int(tile_size[0]), int(tile_size[1])
        self.ntx, self.nty = ceildiv(self.img_w, self.tile_w), ceildiv(self.img_h, self.tile_h)
        self.num_tiles = self.ntx * self.nty
        self.requested_waves = int(waves)
        self.max_wave_idx = 0
        self._job_idx = 0
        self._force_stop = False
        self._lock = threading.Lock()
        self._start = time.monotonic()

    # token next() without per-tile wave gating: on the GPU two waves of a tile may be in flight together
    # (the reference serialises them, tile_provider.cpp:40-60) -- the ordered film (the default) stores every
    # sample and adds them pixel by pixel in wave order after the launch; VPT_FILM_ATOMIC adds with fp32 atomics.
    def next_batch(self, max_jobs: int):
        """Reserve up to max_jobs consecutive job ids: (jid_begin, count), count 0 when done."""
        with self._lock:
            if self._force_stop:
                return self._job_idx, 0
            end = self.requested_waves * self.num_tiles
            begin = self._job_idx
            count = max(0, min(max_jobs, end - begin))
            self._job_idx += count
            if count:
                self.max_wave_idx = max(self.max_wave_idx, 1 + (begin + count - 1) // self.num_tiles)
            return begin, count

    def job(self, jid: int):
        """(tile, wave) of a job id (tile_provider.cpp:30-31)."""
        return jid % self.num_tiles, 1 + jid // self.num_tiles

    def compute_tile_rect(self, tile: int):
        """tile_provider.cpp:95-105 -> (x0, y0, w, h)."""
        x0 = (tile % self.ntx) * self.tile_w
        y0 = (tile // self.ntx) * self.tile_h
        return x0, y0, min(self.img_w - x0, self.tile_w), min(self.img_h - y0, self.tile_h)

    def stop_at_next_wave(self):
        """tile_provider.cpp:107-110: requested_waves = the highest wave already started."""
        with self._lock:
            self.requested_waves = self.max_wave_idx

    def stop_now(self):
        self._force_stop = True

    def reset_eta(self):
        self._start = time.monotonic()

    def progress_ratio(self) -> float:
        total = self.requested_waves * self.num_tiles
        return self._job_idx / total if total else 1.0

    def progress(self) -> int:
        return int(self.progress_ratio() * 100.0)

    def eta(self) -> float:
        p = self.progress_ratio()
        el = time.monotonic() - self._start
        return (1 - p) / (p / el) if p > 0 and el > 0 else float("inf")


class Integrator:
    """One HIP context on one device: the flattened grids, scene constants and a film."""

    def __init__(self, cfg: capi.Configuration, density, temperature=None, device: int = 0, blackbody=None):
        import torch

        self.torch = torch
        self.cfg = cfg.copy()
        self.device = int(device)
        self.dev = torch.device("cuda", self.device)
        L = capi.lib()
        h = C.c_void_p()
        dens_desc = density.desc if hasattr(density, "desc") else density
        temp_desc = None if temperature is None else (temperature.desc if hasattr(temperature, "desc") else temperature)
        bb = None
        if blackbody is not None:
            bb = np.ascontiguousarray(blackbody, np.float32)
        capi.check(L.vpt_gpu_create(C.byref(self.cfg), C.byref(dens_desc),
                                    C.byref(temp_desc) if temp_desc is not None else None,
                                    bb.ctypes.data_as(C.POINTER(C.c_float)) if bb is not None else None,
                                    self.device, C.byref(h)), "vpt_gpu_create")
        self._attach(h)

    def _attach(self, h) -> None:
        self.h = h
        jpw, tot = C.c_uint64(), C.c_uint64()
        capi.check(capi.lib().vpt_gpu_job_space(h, C.byref(jpw), C.byref(tot)), "vpt_gpu_job_space")
        self.jobs_per_wave, self.total_jobs = int(jpw.value), int(tot.value)
        self.film = self.torch.zeros((self.cfg.height, self.cfg.width, 4), dtype=self.torch.float32, device=self.dev)

    @classmethod
    def create_many(cls, cfg: capi.Configuration, density, temperature=None, devices=(0,)) -> list:
        """One Integrator per device with the grids flattened once (vpt_gpu_create_many, what the multi-GPU drop-in
        uses); devices may repeat (several contexts on one GPU)."""
        import torch

        L = capi.lib()
        dens_desc = density.desc if hasattr(density, "desc") else density
        temp_desc = None if temperature is None else (temperature.desc if hasattr(temperature, "desc") else temperature)
        n = len(devices)
        devs = (C.c_int * n)(*[int(d) for d in devices])
        hs = (C.c_void_p * n)()
        cfg_c = cfg.copy()
        capi.check(L.vpt_gpu_create_many(C.byref(cfg_c), C.byref(dens_desc),
                                         C.byref(temp_desc) if temp_desc is not None else None, None, devs, n, hs),
                   "vpt_gpu_create_many")
        out = []
        for d, h in zip(devices, hs):
            it = cls.__new__(cls)
            it.torch, it.cfg, it.device = torch, cfg.copy(), int(d)
            it.dev = torch.device("cuda", it.device)
            it._attach(C.c_void_p(h))
            out.append(it)
        return out

    def setup_timings(self) -> dict:
        """vpt_gpu_setup_timings (ms): flatten + majorant fix, upload, the rest, tile costs, device bind."""
        ms = (C.c_double * 5)()
        capi.check(capi.lib().vpt_gpu_setup_timings(self.h, ms, 5), "vpt_gpu_setup_timings")
        return dict(zip(("flatten_fix", "upload", "rest", "tile_costs", "bind"), (float(x) for x in ms)))

    # ---- sequences: in-place updates (include/vpt_gpu.h "sequences") -------------------------------------------
    def _refresh(self, cfg: capi.Configuration) -> None:
        self.cfg = cfg
        jpw, tot = C.c_uint64(), C.c_uint64()
        capi.check(capi.lib().vpt_gpu_job_space(self.h, C.byref(jpw), C.byref(tot)), "vpt_gpu_job_space")
        self.jobs_per_wave, self.total_jobs = int(jpw.value), int(tot.value)

    def set_scene(self, cfg: capi.Configuration) -> None:
        """Replace the configuration in place (vpt_gpu_set_scene): everything but output_size and tile_size may
        change.  Synchronous; the next frame equals a fresh Integrator's for `cfg`, byte for byte.  Tuning, RNG mode,
        pool layout, film and job order settings stay; tile costs (computed or set) and a job permutation are
        dropped.  self.film is kept (not cleared).  On an error the Integrator renders its previous scene."""
        c = cfg.copy()
        capi.check(capi.lib().vpt_gpu_set_scene(self.h, C.byref(c)), "vpt_gpu_set_scene")
        self._refresh(c)

    def set_camera(self, position=None, look=None, up=None, vfov_deg=None) -> None:
        """set_scene with the camera fields given replaced (the others, and the rest of the scene, as they are)."""
        from .scenes import with_camera

        self.set_scene(with_camera(self.cfg, position, look, up, vfov_deg))

    def set_volume(self, density, temperature=None) -> None:
        """Replace the volume in place (vpt_grids_flatten + vpt_gpu_set_grids); the configuration stays.  A
        temperature grid must be given exactly if the Integrator was created with one.  Synchronous.  If the swap
        fails after the old volume was freed the Integrator has no volume until a later set_volume succeeds (every
        render raises, VPT_E_STATE)."""
        L = capi.lib()
        dens_desc = density.desc if hasattr(density, "desc") else density
        temp_desc = None if temperature is None else (temperature.desc if hasattr(temperature, "desc") else temperature)
        g = C.c_void_p()
        capi.check(L.vpt_grids_flatten(C.byref(dens_desc), C.byref(temp_desc) if temp_desc is not None else None,
                                       C.byref(g)), "vpt_grids_flatten")
        try:
            capi.check(L.vpt_gpu_set_grids(self.h, g), "vpt_gpu_set_grids")
        finally:
            L.vpt_grids_free(g)
        self._refresh(self.cfg)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                capi.lib().vpt_gpu_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def stream_handle(self, stream=None) -> int:
        s = stream if stream is not None else self.torch.cuda.current_stream(self.dev)
        return int(s.cuda_stream)

    def render_jobs(self, jid_begin: int, jid_count: int, film=None, records=None, stream=None):
        """Asynchronously render jobs [jid_begin, jid_begin + jid_count) into `film` (default: own)."""
        film = self.film if film is None else film
        assert film.is_cuda and film.dtype == self.torch.float32 and film.is_contiguous()
        assert film.numel() == self.cfg.height * self.cfg.width * 4
        L = capi.lib()
        s = C.c_void_p(self.stream_handle(stream))
        if records is None:
            capi.check(L.vpt_gpu_render_jobs(self.h, jid_begin, jid_count, C.c_void_p(film.data_ptr()), s),
                       "vpt_gpu_render_jobs")
        else:
            area = int(self.cfg.tile_size[0] * self.cfg.tile_size[1])
            assert records.numel() >= jid_count * area * 3 and records.dtype == self.torch.float32
            capi.check(L.vpt_gpu_render_jobs_records(self.h, jid_begin, jid_count, C.c_void_p(film.data_ptr()),
                                                     C.c_void_p(records.data_ptr()), s),
                       "vpt_gpu_render_jobs_records")

    def render_waves(self, first_wave: int, num_waves: int, film=None, stream=None):
        """Waves are 1-based (tile_provider.cpp:30): wave w covers jids [(w-1)*T, w*T)."""
        self.render_jobs((first_wave - 1) * self.jobs_per_wave, num_waves * self.jobs_per_wave, film, None, stream)

    def render_tiles(self, tile_lo: int, tile_hi: int, first_wave: int, num_waves: int, film=None, stream=None):
        """Asynchronously render waves first_wave .. first_wave + num_waves - 1 (1-based, as render_waves) of the
        tiles [tile_lo, tile_hi) into `film` (default: own) with one band launch (vpt_gpu_render_tiles): the band's
        pixels receive their samples in wave order, bit for bit the reference's film, and no other pixel is
        touched -- so films of disjoint bands sum exactly.  Needs the ordered film (the default)."""
        film = self.film if film is None else film
        assert film.is_cuda and film.dtype == self.torch.float32 and film.is_contiguous()
        assert film.numel() == self.cfg.height * self.cfg.width * 4
        if first_wave < 1 or num_waves < 0:
            raise ValueError("render_tiles: waves are 1-based, num_waves >= 0")
        if not (0 <= tile_lo <= 0xFFFFFFFF and 0 <= tile_hi <= 0xFFFFFFFF):
            raise ValueError("render_tiles: tile indices are 32-bit")
        capi.check(capi.lib().vpt_gpu_render_tiles(self.h, int(tile_lo), int(tile_hi), int(first_wave) - 1,
                                                   int(num_waves), C.c_void_p(film.data_ptr()),
                                                   C.c_void_p(self.stream_handle(stream))), "vpt_gpu_render_tiles")

    def _check_plane(self, m2) -> None:
        assert m2.is_cuda and m2.dtype == self.torch.float32 and m2.is_contiguous()
        assert m2.numel() == self.cfg.height * self.cfg.width

    def set_film_moments(self, m2) -> None:
        """Attach a second-moment plane (a device float32 [H][W] tensor; None detaches): while attached, the ordered
        film passes also add (imaging_ratio * L.y)^2 of every sample into it, in wave order
        (vpt_gpu_set_film_moments).  The tensor is kept alive while it is attached."""
        if m2 is not None:
            self._check_plane(m2)
        capi.check(capi.lib().vpt_gpu_set_film_moments(self.h, C.c_void_p(m2.data_ptr()) if m2 is not None else None),
                   "vpt_gpu_set_film_moments")
        self._m2 = m2

    def set_light_groups(self, groups) -> None:
        """Attach light-group planes (a device float32 [3][H][W][4] tensor -- emission, sun, sky, each an XYZW film;
        None detaches): while attached, the ordered film passes also add every sample's emission, distant-light and
        infinite-light terms into them, in wave order (vpt_gpu_set_light_groups).  Each plane is the film the
        reference renders with the other two sources off.  The tensor is kept alive while it is attached."""
        if groups is not None:
            assert groups.is_cuda and groups.dtype == self.torch.float32 and groups.is_contiguous()
            assert tuple(groups.shape) == (3, self.cfg.height, self.cfg.width, 4)
        capi.check(capi.lib().vpt_gpu_set_light_groups(self.h, C.c_void_p(groups.data_ptr()) if groups is not None else None),
                   "vpt_gpu_set_light_groups")
        self._groups = groups

    def set_shutter(self, cameras) -> None:
        """Attach a shutter (vpt_gpu_set_shutter): a list of 1 .. 65536 cameras, each a dict of the keywords set_camera
        takes (position, look, up, vfov_deg; an absent key keeps the scene's value); None or an empty list detaches.
        While attached, wave w of render_jobs / render_waves, render_tiles and render_tile_list -- so render_uniform and
        render_adaptive's rounds driver too -- generates its primary rays through camera (w - 1) % len(cameras) (waves
        are 1-based here); no random draw changes.  scenes.shutter_cameras makes the list for a camera move.
        Synchronous.  A camera that is not one (look == position, ...) raises and leaves the previous shutter."""
        from .scenes import shutter_entries

        arr = shutter_entries(self.cfg, cameras) if cameras else None
        capi.check(capi.lib().vpt_gpu_set_shutter(self.h, arr, len(arr) if arr is not None else 0), "vpt_gpu_set_shutter")

    def shutter_info(self) -> int:
        """The number of cameras of the attached shutter, 0 if none."""
        n = C.c_uint32()
        capi.check(capi.lib().vpt_gpu_shutter_info(self.h, C.byref(n)), "vpt_gpu_shutter_info")
        return int(n.value)

    def relight(self, groups, gains, stream=None):
        """The relit film [H][W][4] of group planes `groups` ([3][H][W][4]) under `gains` (3 x 3, [group][XYZ]; see
        scenes.light_gains): out.c = ((G0.c k0.c) + (G1.c k1.c)) + (G2.c k2.c), out.w = G0.w, by one small kernel
        (vpt_gpu_relight; image.relight is the same arithmetic in numpy).  Takes a device tensor or a numpy array and
        returns the same kind, as denoise does; with a tensor the call is asynchronous on `stream`."""
        torch = self.torch
        as_numpy = not torch.is_tensor(groups)
        H, W = self.cfg.height, self.cfg.width
        k = np.ascontiguousarray(np.asarray(gains, dtype=np.float32).reshape(-1))
        if k.size != 9:
            raise ValueError("relight: gains is 3 x 3, [group][XYZ]")
        s = stream if stream is not None else torch.cuda.current_stream(self.dev)
        with torch.cuda.stream(s):
            g = groups if not as_numpy else torch.from_numpy(np.array(groups, dtype=np.float32, order="C"))
            g = g.to(device=self.dev, dtype=torch.float32).contiguous()
            if tuple(g.shape) != (3, H, W, 4):
                raise ValueError(f"relight: expected planes of shape {(3, H, W, 4)}, got {tuple(g.shape)}")
            out = torch.empty((H, W, 4), dtype=torch.float32, device=self.dev)
        capi.check(capi.lib().vpt_gpu_relight(self.h, C.c_void_p(g.data_ptr()), k.ctypes.data_as(C.POINTER(C.c_float)),
                                              C.c_void_p(out.data_ptr()), C.c_void_p(int(s.cuda_stream))),
                   "vpt_gpu_relight")
        if as_numpy:
            s.synchronize()
            return out.cpu().numpy()
        return out

    def render_tile_list(self, tiles, first_wave: int, num_waves: int, film=None, stream=None):
        """render_tiles for an arbitrary list of tiles (strictly ascending indices < T) with one list launch
        (vpt_gpu_render_tile_list); waves are 1-based, as render_tiles."""
        film = self.film if film is None else film
        assert film.is_cuda and film.dtype == self.torch.float32 and film.is_contiguous()
        assert film.numel() == self.cfg.height * self.cfg.width * 4
        if first_wave < 1 or num_waves < 0:
            raise ValueError("render_tile_list: waves are 1-based, num_waves >= 0")
        t = np.asarray(tiles, dtype=np.int64).reshape(-1)
        if t.size and (t.min() < 0 or t.max() > 0xFFFFFFFF):
            raise ValueError("render_tile_list: tile indices are 32-bit")
        t = np.ascontiguousarray(t, np.uint32)
        capi.check(capi.lib().vpt_gpu_render_tile_list(self.h, t.ctypes.data_as(C.POINTER(C.c_uint32)), int(t.size),
                                                       int(first_wave) - 1, int(num_waves), C.c_void_p(film.data_ptr()),
                                                       C.c_void_p(self.stream_handle(stream))), "vpt_gpu_render_tile_list")

    def tile_errors(self, m2, film=None, abs_floor: float = 1e-3, stream=None) -> np.ndarray:
        """Per-tile error estimates float32[T] of `film` (default: own) and its moment plane `m2`
        (vpt_gpu_tile_errors: the tile's mean standard error of Y over its mean Y); synchronous."""
        film = self.film if film is None else film
        assert film.is_cuda and film.dtype == self.torch.float32 and film.is_contiguous()
        assert film.numel() == self.cfg.height * self.cfg.width * 4
        self._check_plane(m2)
        err = np.zeros(self.cfg.jobs_per_wave(), np.float32)
        capi.check(capi.lib().vpt_gpu_tile_errors(self.h, C.c_void_p(film.data_ptr()), C.c_void_p(m2.data_ptr()),
                                                  float(abs_floor), err.ctypes.data_as(C.POINTER(C.c_float)),
                                                  C.c_void_p(self.stream_handle(stream))), "vpt_gpu_tile_errors")
        return err

    def render_alpha(self, sub=None, tau: bool = False, stream=None):
        """The coverage matte, numpy float32 [H][W]: alpha = 1 - mean exp(-optical depth) over sub x sub sub-rays of
        each pixel's jitter footprint, by one deterministic pass (vpt_gpu_render_alpha: no random numbers, no
        noise).  sub=None: 4 with jitter, 1 without (all sub-rays coincide then).  tau=True: (alpha, tau) with the
        mean optical depth plane.  Synchronous (the planes are read back); in single-pixel mode every other pixel
        is 0.  Touches no film."""
        torch = self.torch
        if sub is None:
            sub = 4 if self.cfg.worker_parameters.use_jitter else 1
        if not 1 <= int(sub) <= 8:
            raise ValueError("render_alpha: sub is 1..8 sub-rays per axis")
        shape = (self.cfg.height, self.cfg.width)
        s = stream if stream is not None else torch.cuda.current_stream(self.dev)
        with torch.cuda.stream(s):  # (the zero fills run on the pass's stream, ahead of it)
            a = torch.zeros(shape, dtype=torch.float32, device=self.dev)
            t = torch.zeros(shape, dtype=torch.float32, device=self.dev) if tau else None
        capi.check(capi.lib().vpt_gpu_render_alpha(self.h, int(sub), C.c_void_p(a.data_ptr()),
                                                   C.c_void_p(t.data_ptr()) if tau else None,
                                                   C.c_void_p(int(s.cuda_stream))), "vpt_gpu_render_alpha")
        s.synchronize()
        return (a.cpu().numpy(), t.cpu().numpy()) if tau else a.cpu().numpy()

    def render_depth(self, opacity=(1.0 / 255.0, 0.5), sub=None, reach: bool = False, stream=None):
        """The depth planes, numpy float32 [K][H][W]: per opacity a_k of `opacity` (1..4 values, 0 < a_0 < ... < 1) the
        distance from the camera at which a pixel's optical depth first reaches -log1p(-a_k), the depth before which
        that fraction of the primary paths has collided, by one deterministic pass (vpt_gpu_render_depth: the matte's
        march, stopped at the last level; no noise); +0.0 where the level is not reached.  sub=None: what it means
        for render_alpha (4 with jitter, 1 without); a pixel holds the mean over the sub-rays that reached the level.
        reach=True: (depth, reach) with the fraction of sub-rays that did.  Synchronous; in single-pixel mode every
        other pixel is 0.  Touches no film."""
        torch = self.torch
        if sub is None:
            sub = 4 if self.cfg.worker_parameters.use_jitter else 1
        if not 1 <= int(sub) <= 8:
            raise ValueError("render_depth: sub is 1..8 sub-rays per axis")
        op = np.ascontiguousarray(np.atleast_1d(np.asarray(opacity, dtype=np.float32)))
        if op.ndim != 1 or not 1 <= op.size <= 4:
            raise ValueError("render_depth: 1..4 opacity levels")
        shape = (int(op.size), self.cfg.height, self.cfg.width)
        s = stream if stream is not None else torch.cuda.current_stream(self.dev)
        with torch.cuda.stream(s):  # (the zero fills run on the pass's stream, ahead of it)
            d = torch.zeros(shape, dtype=torch.float32, device=self.dev)
            r = torch.zeros(shape, dtype=torch.float32, device=self.dev) if reach else None
        capi.check(capi.lib().vpt_gpu_render_depth(self.h, int(sub), int(op.size), op.ctypes.data_as(C.POINTER(C.c_float)),
                                                   C.c_void_p(d.data_ptr()), C.c_void_p(r.data_ptr()) if reach else None,
                                                   C.c_void_p(int(s.cuda_stream))), "vpt_gpu_render_depth")
        s.synchronize()
        return (d.cpu().numpy(), r.cpu().numpy()) if reach else d.cpu().numpy()

    def denoise(self, film, m2, guides=(), guide_sigma=None, iterations: int = 4, sigma_l: float = 4.0,
                rel_floor: float = 1e-3, variance: bool = False, stream=None):
        """The denoised film of `film` ([H][W][4]) and its moment plane `m2` ([H][W]): the variance-guided a-trous
        filter of vpt_gpu_denoise, guided by up to four planes `guides` ([H][W] each; render.matte_guides gives the
        matte's two) with scale `guide_sigma` (None: 0.2 per guide; a number: that for each; or one per guide).
        Takes device tensors or numpy arrays and returns the same kind (what `film` is); variance=True: (film, var)
        with the filtered variance of the mean of Y.  The inputs are not changed; the result is an ordinary film.
        With tensors the call is asynchronous on `stream` (default: the current one), and the tensors must be ready
        on that stream: what another stream produced has to be ordered before the call by the caller (an event or a
        synchronize).  numpy inputs are uploaded on `stream` itself.  Calls on different streams of one Integrator are
        safe: the library runs them one after the other (they share the context's packed planes)."""
        torch = self.torch
        as_numpy = not torch.is_tensor(film)
        if not 1 <= int(iterations) <= 6:
            raise ValueError("denoise: iterations is 1..6")
        guides = list(guides)
        if len(guides) > 4:
            raise ValueError("denoise: at most 4 guides")
        H, W = self.cfg.height, self.cfg.width
        s = stream if stream is not None else torch.cuda.current_stream(self.dev)

        def dev(a, shape):
            t = a if torch.is_tensor(a) else torch.from_numpy(np.array(a, dtype=np.float32, order="C"))  # (a copy)
            t = t.to(device=self.dev, dtype=torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"denoise: expected a plane of shape {shape}, got {tuple(t.shape)}")
            return t

        with torch.cuda.stream(s):
            f, m = dev(film, (H, W, 4)), dev(m2, (H, W))
            gs = [dev(g, (H, W)) for g in guides]
            out = torch.empty_like(f)
            var = torch.empty_like(m) if variance else None
        p = capi.DenoiseParams.make(iterations, len(gs), sigma_l, rel_floor, guide_sigma)
        gp = (C.c_void_p * max(1, len(gs)))(*[g.data_ptr() for g in gs])
        capi.check(capi.lib().vpt_gpu_denoise(self.h, C.byref(p), C.c_void_p(f.data_ptr()), C.c_void_p(m.data_ptr()),
                                              gp if gs else None, C.c_void_p(out.data_ptr()),
                                              C.c_void_p(var.data_ptr()) if variance else None,
                                              C.c_void_p(int(s.cuda_stream))), "vpt_gpu_denoise")
        if as_numpy:
            s.synchronize()
            return (out.cpu().numpy(), var.cpu().numpy()) if variance else out.cpu().numpy()
        return (out, var) if variance else out

    def temporal(self, film, m2, depth, prev_camera, history=None, max_history=None, depth_tol: float = 0.1,
                 sigma_r: float = 4.0, rel_floor: float = 1e-3, motion: bool = False, hist_n: bool = False, stream=None,
                 out=None):
        """`film` ([H][W][4]) and its moment plane `m2` ([H][W]) with the previous frame's accumulated film added
        (vpt_gpu_temporal): `history` = (film, m2, depth) of the previous frame is reprojected through this frame's
        depth planes `depth` ([K][H][W], what render_depth returns; sub=1) from the Integrator's current camera into
        `prev_camera`, the camera the history was rendered with (a dict of set_camera's keywords; an absent key keeps
        the scene's value).  history=None: the film and plane pass through.  max_history caps the history's sample
        count per pixel (None: 4 * cfg.num_waves); depth_tol is the relative depth tolerance of a history tap; sigma_r
        and rel_floor scale the rejection on Y.  -> (film, m2), an ordinary film and plane (the next frame's history,
        with `depth` and the current camera); motion=True / hist_n=True append the motion plane ([H][W][2], pixels the
        point moved from this frame's raster to the previous one's; NaN where it has no projection) and the history
        count added per pixel ([H][W]).  Takes device tensors or numpy arrays and returns the same kind (what `film`
        is); the inputs are not changed.  With tensors the call is asynchronous on `stream` (default: the current
        one).  out: (film, m2) device tensors to write instead of new ones (render.TemporalState's buffers)."""
        from .scenes import shutter_entries

        torch = self.torch
        as_numpy = not torch.is_tensor(film)
        H, W = self.cfg.height, self.cfg.width
        s = stream if stream is not None else torch.cuda.current_stream(self.dev)
        cam = shutter_entries(self.cfg, [dict(prev_camera)])

        def dev(a, shape):
            t = a if torch.is_tensor(a) else torch.from_numpy(np.array(a, dtype=np.float32, order="C"))  # (a copy)
            t = t.to(device=self.dev, dtype=torch.float32).contiguous()
            if shape[0] is None:
                shape = (t.shape[0] if t.dim() == 3 else -1,) + shape[1:]
            if tuple(t.shape) != shape:
                raise ValueError(f"temporal: expected a plane of shape {shape}, got {tuple(t.shape)}")
            return t

        with torch.cuda.stream(s):
            f, m, d = dev(film, (H, W, 4)), dev(m2, (H, W)), dev(depth, (None, H, W))
            K = int(d.shape[0])
            if not 1 <= K <= 4:
                raise ValueError("temporal: 1..4 depth planes")
            hf = hm = hd = None
            if history is not None:
                hf, hm, hd = history
                hf, hm, hd = dev(hf, (H, W, 4)), dev(hm, (H, W)), dev(hd, (K, H, W))
            of, om = (torch.empty_like(f), torch.empty_like(m)) if out is None else out
            mv = torch.empty((H, W, 2), dtype=torch.float32, device=self.dev) if motion else None
            hn = torch.empty((H, W), dtype=torch.float32, device=self.dev) if hist_n else None
        if max_history is None:
            max_history = 4 * int(self.cfg.num_waves)
        p = capi.TemporalParams.make(K, max_history, depth_tol, sigma_r, rel_floor)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        capi.check(capi.lib().vpt_gpu_temporal(self.h, C.byref(p), ptr(f), ptr(m), ptr(d), cam, ptr(hf), ptr(hm), ptr(hd),
                                               ptr(of), ptr(om), ptr(mv), ptr(hn), C.c_void_p(int(s.cuda_stream))),
                   "vpt_gpu_temporal")
        res = (of, om) + ((mv,) if motion else ()) + ((hn,) if hist_n else ())
        if as_numpy:
            s.synchronize()
            return tuple(t.cpu().numpy() for t in res)
        return res

    def trace_jobs(self, jid_begin: int, jid_count: int, capacity: int = 1 << 20, film=None, stream=None):
        """Render jobs and return their Logger events (worker.cpp:16-48) as a numpy array of
        capi.EVENT_DTYPE sorted by (jid, seq).  Raises if more than `capacity` events occur."""
        torch = self.torch
        film = self.film if film is None else film
        buf = torch.empty((max(1, capacity), capi.EVENT_DTYPE.itemsize), dtype=torch.uint8, device=self.dev)
        n = C.c_uint64()
        capi.check(capi.lib().vpt_gpu_trace_jobs(self.h, jid_begin, jid_count, C.c_void_p(film.data_ptr()),
                                                 C.c_void_p(buf.data_ptr()), capacity, C.byref(n),
                                                 C.c_void_p(self.stream_handle(stream))), "vpt_gpu_trace_jobs")
        if n.value > capacity:
            raise RuntimeError(f"trace_jobs: {n.value} events exceed capacity {capacity}")
        ev = buf[: n.value].cpu().numpy().view(capi.EVENT_DTYPE).reshape(-1)
        return np.sort(ev, order=["jid", "seq"])

    def majorant_trace(self, origin, direction, max_rows: int = 1 << 16) -> np.ndarray:
        """Volume::log_majorant_trace (volume.cpp:176-192) rows [n][9] for one world ray."""
        o = np.ascontiguousarray(origin, np.float32).reshape(3)
        d = np.ascontiguousarray(direction, np.float32).reshape(3)
        rows = np.zeros((max_rows, 9), np.float32)
        n = C.c_int()
        fp = C.POINTER(C.c_float)
        capi.check(capi.lib().vpt_gpu_majorant_trace(self.h, o.ctypes.data_as(fp), d.ctypes.data_as(fp),
                                                     rows.ctypes.data_as(fp), max_rows, C.byref(n)),
                   "vpt_gpu_majorant_trace")
        if n.value > max_rows:
            raise RuntimeError(f"majorant_trace: {n.value} segments exceed max_rows {max_rows}")
        return rows[: n.value].copy()

    def set_rng_mode(self, mode: int) -> None:
        """capi.VPT_RNG_REFERENCE (default, the reference's samples) or capi.VPT_RNG_PIXEL
        (throughput mode: one stream per pixel; matches the reference only in expectation)."""
        capi.check(capi.lib().vpt_gpu_set_rng_mode(self.h, int(mode)), "vpt_gpu_set_rng_mode")

    def set_pixel_chunk(self, chunk: int) -> None:
        """Throughput mode: pixels per work item (0 = auto; else a power of two dividing the tile area).
        Samples never depend on it."""
        capi.check(capi.lib().vpt_gpu_set_pixel_chunk(self.h, int(chunk)), "vpt_gpu_set_pixel_chunk")

    def set_run_skipping(self, mode: int) -> None:
        """-1: the creation-time choice; 0 / 1: force the run-skipping kernel variant off / on."""
        capi.check(capi.lib().vpt_gpu_set_run_skipping(self.h, int(mode)), "vpt_gpu_set_run_skipping")

    def set_latency_kernel(self, mode: int, ungated: int = -1) -> None:
        """The latency kernel (lane cold state in VGPRs, 4-5 waves per SIMD): -1 auto (latency-bound launches,
        C1, and partly filled ones, C2 and small shares), 0 never, 1 always; `ungated` 1 / 0: partly filled
        launches on it use the latency gates / the context's (-1 keeps; default 0).  Samples never depend on it."""
        capi.check(capi.lib().vpt_gpu_set_latency_kernel(self.h, int(mode), int(ungated)), "vpt_gpu_set_latency_kernel")

    def set_compaction(self, every: int) -> None:
        """Live-path compaction on partly filled latency launches every `every` outer iterations (0: off);
        see include/vpt_gpu.h vpt_gpu_set_compaction.  Samples never depend on it."""
        capi.check(capi.lib().vpt_gpu_set_compaction(self.h, int(every)), "vpt_gpu_set_compaction")

    def latency_kernel_info(self) -> dict:
        m, b = C.c_int(), C.c_int()
        capi.check(capi.lib().vpt_gpu_latency_kernel_info(self.h, C.byref(m), C.byref(b)), "vpt_gpu_latency_kernel_info")
        return {"mode": int(m.value), "resident_blocks_per_cu": int(b.value)}

    def kernel_variant(self, last_launch: bool = False) -> dict:
        """The production kernel this context launches.  last_launch: also what the last launch ran -- `eval_split`,
        True when its instantiation evaluates densities in two halves (None before the first launch)."""
        t, r = C.c_int(), C.c_int()
        capi.check(capi.lib().vpt_gpu_kernel_variant(self.h, C.byref(t), C.byref(r)), "vpt_gpu_kernel_variant")
        kv = {"has_temperature": bool(t.value), "run_skipping": bool(r.value)}
        if last_launch:
            e = C.c_int()
            capi.check(capi.lib().vpt_gpu_last_launch_variant(self.h, C.byref(e)), "vpt_gpu_last_launch_variant")
            kv["eval_split"] = None if e.value < 0 else bool(e.value)
        return kv

    def set_film_order(self, mode: int, max_bytes: int = 0) -> None:
        """capi.VPT_FILM_ORDERED (default: every pixel's samples added in wave order, the reference's film bit
        for bit; `max_bytes` caps the sample buffer, 0 = auto) or capi.VPT_FILM_ATOMIC (fp32 atomics in
        completion order).  See include/vpt_gpu.h vpt_gpu_set_film_order."""
        capi.check(capi.lib().vpt_gpu_set_film_order(self.h, int(mode), int(max_bytes)), "vpt_gpu_set_film_order")

    def film_order_info(self) -> dict:
        m, b, o, a = C.c_int(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        capi.check(capi.lib().vpt_gpu_film_order_info(self.h, C.byref(m), C.byref(b), C.byref(o), C.byref(a)),
                   "vpt_gpu_film_order_info")
        return {"mode": int(m.value), "buffer_bytes": int(b.value), "ordered_launches": int(o.value),
                "atomic_launches": int(a.value)}

    def set_pool_layout(self, layout: int, cap_bytes: int | None = None) -> None:
        """capi.VPT_POOL_AUTO (default: the direct-addressed stencil pool when it fits the cap), VPT_POOL_DENSE or
        VPT_POOL_SPARSE; `cap_bytes` sets VPT_POOL_AUTO's cap first (0 = 1/8 of the device's memory).  Results never
        depend on it.  See include/vpt_gpu.h vpt_gpu_set_pool_layout."""
        if cap_bytes is not None:
            capi.check(capi.lib().vpt_gpu_set_pool_cap(self.h, int(cap_bytes)), "vpt_gpu_set_pool_cap")
        capi.check(capi.lib().vpt_gpu_set_pool_layout(self.h, int(layout)), "vpt_gpu_set_pool_layout")

    def pool_info(self) -> dict:
        """The stencil pool's layout in use, the policy, and both pools' bytes as (density, temperature)."""
        la, po, ms = C.c_int(), C.c_int(), C.c_double()
        sp, de = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
        capi.check(capi.lib().vpt_gpu_pool_info(self.h, C.byref(la), C.byref(po), sp, de, C.byref(ms)), "vpt_gpu_pool_info")
        return {"layout": int(la.value), "policy": int(po.value), "sparse_bytes": (int(sp[0]), int(sp[1])),
                "dense_bytes": (int(de[0]), int(de[1])), "expand_ms": float(ms.value)}

    def debug_read_pool(self, grid: int, cell_begin: int, cell_count: int) -> np.ndarray:
        """Debug (tests): the dense bricks of table cells [cell_begin, + cell_count) as float32[cell_count, 2304]."""
        out = np.empty((int(cell_count), 2304), dtype=np.float32)
        capi.check(capi.lib().vpt_gpu_debug_read_pool(self.h, int(grid), int(cell_begin), int(cell_count),
                                                      out.ctypes.data_as(C.POINTER(C.c_float))), "vpt_gpu_debug_read_pool")
        return out

    def set_job_order(self, mode: int) -> None:
        """Scheduling order of whole-wave launches: capi.VPT_ORDER_JID (TileProvider order),
        VPT_ORDER_COST_WAVE_MAJOR, VPT_ORDER_COST_TILE_MAJOR, VPT_ORDER_COST_TAIL or VPT_ORDER_COST_SAME_TILE
        (default; launches that add with film atomics take VPT_ORDER_COST_TAIL).
        Samples never depend on it."""
        capi.check(capi.lib().vpt_gpu_set_job_order(self.h, int(mode)), "vpt_gpu_set_job_order")

    def set_job_order_tail(self, waves: int) -> None:
        """VPT_ORDER_COST_TAIL's tile-major wave count (0 = auto)."""
        capi.check(capi.lib().vpt_gpu_set_job_order_tail(self.h, int(waves)), "vpt_gpu_set_job_order_tail")

    def tile_costs(self):
        """(cost float32[T], tile ranks by descending cost uint32[T]) of the job-order pass."""
        T = self.cfg.jobs_per_wave()
        cost, rank = np.zeros(T, np.float32), np.zeros(T, np.uint32)
        capi.check(capi.lib().vpt_gpu_tile_costs(self.h, cost.ctypes.data_as(C.POINTER(C.c_float)),
                                                  rank.ctypes.data_as(C.POINTER(C.c_uint32))), "vpt_gpu_tile_costs")
        return cost, rank

    def set_tile_costs(self, cost) -> None:
        """Replace the job-order cost estimates with per-tile costs (float32[T], e.g. measured)."""
        c = np.ascontiguousarray(cost, np.float32)
        assert c.shape == (self.cfg.jobs_per_wave(),)
        capi.check(capi.lib().vpt_gpu_set_tile_costs(self.h, c.ctypes.data_as(C.POINTER(C.c_float))),
                   "vpt_gpu_set_tile_costs")

    def set_job_permutation(self, perm) -> None:
        """Explicit order of launches with len(perm) jobs: item k renders job jid_begin + perm[k]
        (None or empty clears it).  Samples never depend on it."""
        p = np.ascontiguousarray(perm if perm is not None else [], np.uint32)
        capi.check(capi.lib().vpt_gpu_set_job_permutation(self.h, p.ctypes.data_as(C.POINTER(C.c_uint32)), p.size),
                   "vpt_gpu_set_job_permutation")

    def job_permutation_size(self) -> int:
        """Length of the explicit job permutation in force (0: none; a scene or volume update drops it)."""
        n = C.c_uint64()
        capi.check(capi.lib().vpt_gpu_job_permutation_info(self.h, C.byref(n)), "vpt_gpu_job_permutation_info")
        return int(n.value)

    def counters(self, reset: bool = False) -> dict:
        c = capi.Counters()
        capi.check(capi.lib().vpt_gpu_counters(self.h, C.byref(c), 1 if reset else 0), "vpt_gpu_counters")
        return c.as_dict()

    def set_tuning(self, gate_min: int = 0, gate_idle: int = -1, grid_blocks: int = 0, gate_eval: int = 0,
                   gate_walk: int = -1):
        capi.check(capi.lib().vpt_gpu_set_tuning(self.h, gate_min, gate_idle, grid_blocks, gate_eval, gate_walk),
                   "vpt_gpu_set_tuning")

    def set_latency_tuning(self, wave_lanes: int = -1, gate_min: int = 0, gate_idle: int = -1, gate_eval: int = 0,
                           gate_walk: int = -1):
        """Knobs of latency-bound launches (fewer items than grid lanes): lanes per wavefront that take
        jobs (0 = auto) and their gates; see include/vpt_gpu.h."""
        capi.check(capi.lib().vpt_gpu_set_latency_tuning(self.h, wave_lanes, gate_min, gate_idle, gate_eval, gate_walk),
                   "vpt_gpu_set_latency_tuning")

    PROFILE_BLOCKS = ["iter", "fetch", "pixel", "ray", "sample", "need_seg", "step", "draw", "trilinear",
                      "event", "shadow_hit", "none", "nee_done", "finish",
                      "w_walk", "w_eval", "w_nee", "w_finish", "w_ray", "w_pixel", "w_done"]

    PROFILE_SECTIONS = ["fetch", "pixel", "ray", "walk", "eval", "nee", "finish", "seg", "step", "draw"]

    def profile(self, reset: bool = False) -> dict:
        """SIMT profile of a -DVPT_PROFILE build: {block: (wave executions, mean active lanes)} and
        {"cycles": {section: share of wave time}}."""
        buf = (C.c_uint64 * 128)()
        capi.check(capi.lib().vpt_gpu_profile(self.h, buf, 128, 1 if reset else 0), "vpt_gpu_profile")
        out = {}
        for i, name in enumerate(self.PROFILE_BLOCKS):
            ex, lanes = int(buf[2 * i]), int(buf[2 * i + 1])
            out[name] = (ex, round(lanes / ex, 2) if ex else 0.0)
        base = 2 * len(self.PROFILE_BLOCKS)
        cyc = [int(buf[base + i]) for i in range(len(self.PROFILE_SECTIONS))]
        tot = sum(cyc) or 1
        out["cycles"] = {n: round(c / tot, 4) for n, c in zip(self.PROFILE_SECTIONS, cyc)}
        out["cycles_total"] = tot
        return out

    def set_full_tuning(self, gate_min: int = 0, gate_idle: int = -1, gate_eval: int = 0, gate_walk: int = -1):
        """Gates of full launches alone (set_tuning writes them and the context's); see include/vpt_gpu.h."""
        capi.check(capi.lib().vpt_gpu_set_full_tuning(self.h, gate_min, gate_idle, gate_eval, gate_walk),
                   "vpt_gpu_set_full_tuning")

    def gate_info(self, gate_set: int):
        """((gate_min, gate_idle, gate_eval, gate_walk) of a gate set (capi.VPT_GATES_*), the set the last launch
        read or -1)."""
        g, last = (C.c_int * 4)(), C.c_int()
        capi.check(capi.lib().vpt_gpu_gate_info(self.h, gate_set, g, C.byref(last)), "vpt_gpu_gate_info")
        return tuple(int(v) for v in g), int(last.value)

    def launch_info(self):
        g, b = C.c_int(), C.c_int()
        capi.check(capi.lib().vpt_gpu_launch_info(self.h, C.byref(g), C.byref(b)), "vpt_gpu_launch_info")
        return int(g.value), int(b.value)

    def film_host(self) -> np.ndarray:
        self.torch.cuda.synchronize(self.dev)
        return self.film.cpu().numpy()


class Feed:
    """A running launch that renders job ids as they are pushed (vpt_gpu_feed_*, include/vpt_gpu.h) into
    `film` (a zeroed device tensor of the context's film shape) on `stream` (a torch stream of the device).  A
    staged feed counts its completed jobs per tile: snapshot() adds what it has rendered so far into a host
    film (also while it runs: the copy engines read the device film beside the launch), collect() the rest
    once it has ended (then it clears `film`)."""

    def __init__(self, integrator: "Integrator", film, stream, window: int = 1 << 19, staged: bool = False):
        self.it, self.film, self.stream = integrator, film, stream
        h = C.c_void_p()
        fn = "vpt_gpu_feed_open_staged" if staged else "vpt_gpu_feed_open"
        capi.check(getattr(capi.lib(), fn)(integrator.h, C.c_void_p(film.data_ptr()),
                                           C.c_void_p(int(stream.cuda_stream)), int(window), C.byref(h)), fn)
        self.h = h

    def push(self, jids) -> None:
        j = np.ascontiguousarray(jids, np.uint64)
        capi.check(capi.lib().vpt_gpu_feed_push(self.h, j.ctypes.data_as(C.POINTER(C.c_uint64)), j.size),
                   "vpt_gpu_feed_push")

    def close(self) -> None:
        capi.check(capi.lib().vpt_gpu_feed_close(self.h), "vpt_gpu_feed_close")

    def done(self) -> bool:
        d = C.c_int()
        capi.check(capi.lib().vpt_gpu_feed_query(self.h, C.byref(d), None), "vpt_gpu_feed_query")
        return bool(d.value)

    def backlog(self) -> int:
        b = C.c_uint64()
        capi.check(capi.lib().vpt_gpu_feed_backlog(self.h, C.byref(b)), "vpt_gpu_feed_backlog")
        return int(b.value)

    def destroy(self) -> None:
        if self.h:
            h, self.h = self.h, None
            capi.check(capi.lib().vpt_gpu_feed_destroy(h), "vpt_gpu_feed_destroy")

    def snapshot(self, film_host: np.ndarray) -> None:
        """Adds what a staged feed has rendered since the previous snapshot into film_host (float32,
        C-contiguous [H][W][4])."""
        assert film_host.dtype == np.float32 and film_host.flags.c_contiguous
        capi.check(capi.lib().vpt_gpu_feed_snapshot(self.h, film_host.ctypes.data_as(C.POINTER(C.c_float))),
                   "vpt_gpu_feed_snapshot")

    def collect(self, film_host: np.ndarray) -> None:
        """Waits for a staged feed and adds the rest of its film into film_host (float32, C-contiguous); frees it."""
        assert film_host.dtype == np.float32 and film_host.flags.c_contiguous
        h, self.h = self.h, None
        capi.check(capi.lib().vpt_gpu_feed_collect(h, film_host.ctypes.data_as(C.POINTER(C.c_float))),
                   "vpt_gpu_feed_collect")


def run(cfg: capi.Configuration, integrator: Integrator, tp: TileProvider, film: Optional[np.ndarray] = None,
        batch_jobs: int = 4096, flush_seconds: float = 0.2, window: int = 1 << 19) -> np.ndarray:
    """Drop-in for vpt::run (worker.cpp:92-208): drain `tp` on the GPU into `film` (host float32 [H][W][4],
    the reference's Image<float,4> layout), as include/vpt_run.hpp's drain does it (without its threads): the
    job ids go to one running launch through a staged feed (no launch drain between batches), every
    flush_seconds what it has completed is added into `film` (vpt_gpu_feed_snapshot) -- which therefore fills
    in during the run (main.cpp:101-132 shows it at 5 FPS) -- and the collect adds the rest."""
    torch = integrator.torch
    out = film if film is not None else np.zeros((integrator.cfg.height, integrator.cfg.width, 4), np.float32)
    if out.dtype != np.float32 or not out.flags.c_contiguous or out.size != integrator.film.numel():
        raise ValueError("run: film must be a C-contiguous float32 [H][W][4] array")
    dev_film = torch.zeros_like(integrator.film)
    torch.cuda.synchronize(integrator.dev)  # zeroed before the feed's launch (on its own stream) reads it
    stream = torch.cuda.Stream(device=integrator.dev)
    feed = Feed(integrator, dev_film, stream, window, staged=True)
    last = time.monotonic()
    try:
        while True:
            begin, count = tp.next_batch(batch_jobs)
            if count == 0:
                break
            feed.push(np.arange(begin, begin + count, dtype=np.uint64))
            if time.monotonic() - last >= flush_seconds:
                feed.snapshot(out)
                last = time.monotonic()
        feed.collect(out)
    finally:
        feed.destroy()
    return out


def render_adaptive(it: Integrator, target_error: float, min_waves: int = 64, step_waves: int = 64,
                    max_waves: Optional[int] = None, abs_floor: float = 1e-3, fused: bool = False,
                    return_moments: bool = False, groups: bool = False):
    """Render a frame from zero until every tile's error estimate (Integrator.tile_errors) is at most
    `target_error` or it has `max_waves` waves (None: cfg.num_waves): `min_waves` waves of every tile, then
    `step_waves` more per round of the tiles still above the target (vpt_gpu_render_adaptive).  Each tile's film
    is the uniform frame's after its own wave count, bit for bit.  fused: the one-launch driver
    (vpt_gpu_render_adaptive_fused: a wavefront owns a tile; the same bytes; tiles of at most 256 pixels).
    -> (film float32[H][W][4], waves uint32[T], err float32[T], info dict); return_moments: the film's moment plane
    (float32[H][W], what Integrator.denoise wants beside the film) is appended.  groups: the frame's light-group planes
    (float32[3][H][W][4], Integrator.set_light_groups) are rendered with it and appended last -- the rounds driver
    only: the fused driver does not write them."""
    torch = it.torch
    if groups and fused:
        raise ValueError("render_adaptive: light groups are rendered by the rounds driver only (fused=False)")
    if fused and hasattr(capi.lib(), "vpt_gpu_shutter_info") and it.shutter_info():  # (older builds in A/B runs lack it)
        raise ValueError("render_adaptive: a shutter is attached and the fused driver does not honour it (fused=False)")
    T = it.cfg.jobs_per_wave()
    film = torch.zeros_like(it.film)
    gp = torch.zeros((3, it.cfg.height, it.cfg.width, 4), dtype=torch.float32, device=it.dev) if groups else None
    m2 = torch.zeros((it.cfg.height, it.cfg.width), dtype=torch.float32, device=it.dev)
    torch.cuda.synchronize(it.dev)
    p = capi.AdaptiveParams(float(target_error), float(abs_floor), int(min_waves), int(step_waves),
                            int(it.cfg.num_waves if max_waves is None else max_waves))
    res = capi.AdaptiveResult()
    waves, err = np.zeros(T, np.uint32), np.zeros(T, np.float32)
    name = "vpt_gpu_render_adaptive_fused" if fused else "vpt_gpu_render_adaptive"
    prev = getattr(it, "_groups", None)
    if groups:
        it.set_light_groups(gp)
    try:
        capi.check(getattr(capi.lib(), name)(it.h, C.byref(p), C.c_void_p(film.data_ptr()), C.c_void_p(m2.data_ptr()),
                                             waves.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             err.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res),
                                             C.c_void_p(it.stream_handle(None))), name)
        torch.cuda.synchronize(it.dev)
    finally:
        if groups:
            it.set_light_groups(prev)
    out = (film.cpu().numpy(), waves, err, res.as_dict())
    if return_moments:
        out += (m2.cpu().numpy(),)
    if groups:
        out += (gp.cpu().numpy(),)
    return out


def render_uniform(it: Integrator, moments: bool = True, groups: bool = False):
    """The whole frame (cfg.num_waves waves of every tile) from zero as one ordered launch -- the reference's film bit
    for bit -- with a moment plane attached: -> (film [H][W][4], m2 [H][W]) device tensors (moments=False: the film
    alone).  groups=True: with light-group planes attached as well (Integrator.set_light_groups), appended as a
    [3][H][W][4] tensor: -> (film, m2, groups).  The context's previous attachments are restored afterwards."""
    torch = it.torch
    film = torch.zeros_like(it.film)
    m2 = torch.zeros((it.cfg.height, it.cfg.width), dtype=torch.float32, device=it.dev) if moments else None
    gp = torch.zeros((3, it.cfg.height, it.cfg.width, 4), dtype=torch.float32, device=it.dev) if groups else None
    torch.cuda.synchronize(it.dev)
    prev, prev_g = getattr(it, "_m2", None), getattr(it, "_groups", None)
    it.set_film_moments(m2)
    if groups:
        it.set_light_groups(gp)
    try:
        it.render_waves(1, int(it.cfg.num_waves), film=film)
        torch.cuda.synchronize(it.dev)
    finally:
        it.set_film_moments(prev)
        if groups:
            it.set_light_groups(prev_g)
    out = (film, m2) if moments else (film,)
    if groups:
        out += (gp,)
    return out if len(out) > 1 else film


def _host_copy(x, torch):
    """x with every device tensor in it (tuples, lists and dicts walked) replaced by a numpy copy."""
    if torch.is_tensor(x):
        return x.detach().cpu().numpy()
    if isinstance(x, tuple):
        return tuple(_host_copy(v, torch) for v in x)
    if isinstance(x, list):
        return [_host_copy(v, torch) for v in x]
    if isinstance(x, dict):
        return {k: _host_copy(v, torch) for k, v in x.items()}
    return x


def render_sequence(it: Integrator, frames, render_frame, sink, depth: int = 2) -> dict:
    """Render a sequence on one Integrator.  `frames` yields (cfg or None, (density, temperature) or None) per frame:
    what changes before it -- the volume first (Integrator.set_volume), then the scene (Integrator.set_scene); (None,
    None) renders the Integrator as it stands.  `render_frame(it)` returns what one frame produces (a film, a tuple of
    planes, ...); device tensors in it are copied to the host here, because the Integrator's buffers serve the next
    frame.  `sink(index, result)` runs on one writer thread behind a queue of `depth` frames, so frame k is converted
    and encoded while frame k + 1 renders; its indices arrive in order.  An exception of the sink ends the sequence
    and is raised here.  -> {"frames", "update_ms": [...], "render_ms": [...], "total_ms"} (update: the two set_ calls;
    render: render_frame and the host copy)."""
    import queue

    q: "queue.Queue" = queue.Queue(maxsize=max(1, int(depth)))
    failed: list = []

    def writer():
        while True:
            item = q.get()
            if item is None:
                return
            if failed:
                continue  # (drain, so that the producer never blocks on a full queue)
            try:
                sink(*item)
            except BaseException as e:  # noqa: BLE001 -- re-raised by the caller's thread
                failed.append(e)

    th = threading.Thread(target=writer, name="vpt-sequence-writer", daemon=True)
    th.start()
    update_ms, render_ms = [], []
    t_begin = time.perf_counter()
    n = 0
    try:
        for cfg, vol in frames:
            if failed:
                break
            t0 = time.perf_counter()
            if vol is not None:
                it.set_volume(*vol)
            if cfg is not None:
                it.set_scene(cfg)
            t1 = time.perf_counter()
            result = _host_copy(render_frame(it), it.torch)
            t2 = time.perf_counter()
            update_ms.append((t1 - t0) * 1e3)
            render_ms.append((t2 - t1) * 1e3)
            q.put((n, result))
            n += 1
    finally:
        q.put(None)
        th.join()
    if failed:
        raise failed[0]
    return {"frames": n, "update_ms": update_ms, "render_ms": render_ms,
            "total_ms": (time.perf_counter() - t_begin) * 1e3}


TEMPORAL_DEPTH_LEVELS = (1.0 / 255.0, 0.5)  # the depth planes a sequence reprojects through (render_depth, sub=1)


class TemporalState:
    """The history of a sequence's temporal accumulation (Integrator.temporal) across the frames of render_sequence:
    two buffer sets (accumulated film, its moment plane, the depth planes) that swap roles every frame -- one is the
    history the pass reads, the other receives its output -- and the camera the history was rendered with.
    accumulate() runs one frame; reset() forgets the history (a cut: the next frame passes through)."""

    def __init__(self, it: Integrator, levels: int = len(TEMPORAL_DEPTH_LEVELS), max_history=None, depth_tol: float = 0.1,
                 sigma_r: float = 4.0, rel_floor: float = 1e-3):
        torch = it.torch
        H, W = it.cfg.height, it.cfg.width
        self.params = dict(max_history=max_history, depth_tol=depth_tol, sigma_r=sigma_r, rel_floor=rel_floor)
        self.sets = [{"film": torch.zeros((H, W, 4), dtype=torch.float32, device=it.dev),
                      "m2": torch.zeros((H, W), dtype=torch.float32, device=it.dev),
                      "depth": torch.zeros((int(levels), H, W), dtype=torch.float32, device=it.dev)} for _ in range(2)]
        self.history = None  # index of the set that holds the history, None before the first frame
        self.camera = None   # the camera that set was rendered with (scenes.camera_of)
        self.frames = 0      # frames accumulated since the last reset

    def reset(self) -> None:
        self.history, self.camera, self.frames = None, None, 0

    def accumulate(self, it: Integrator, film, m2, depth=None, motion: bool = False, hist_n: bool = False):
        """One frame: `film` and `m2` (the frame as rendered) plus the history -> the accumulated (film, m2[, motion]
        [, hist_n]): numpy arrays for numpy inputs, else device tensors -- the state's own buffers, which stay valid
        until the frame after the next.  depth: this
        frame's depth planes (numpy or tensor; None: render_depth(TEMPORAL_DEPTH_LEVELS, sub=1) here).  The output,
        the depth planes and the Integrator's camera then become the history."""
        from .scenes import camera_of

        if depth is None:
            depth = it.render_depth(TEMPORAL_DEPTH_LEVELS, sub=1)
        out = self.sets[1 if self.history == 0 else 0]
        hist = self.sets[self.history] if self.history is not None else None
        out["depth"].copy_(it.torch.as_tensor(depth, dtype=it.torch.float32))
        cam = camera_of(it.cfg)
        res = it.temporal(film, m2, out["depth"], self.camera if hist is not None else cam,
                          None if hist is None else (hist["film"], hist["m2"], hist["depth"]), motion=motion, hist_n=hist_n,
                          out=(out["film"], out["m2"]), **self.params)
        self.history, self.camera = (1 if self.history == 0 else 0), cam
        self.frames += 1
        return res


def matte_guides(it: Integrator, sub: int = 1):
    """The denoiser's two guide planes of a volume, numpy float32 [H][W] each, from one coverage pass
    (render_alpha(sub, tau=True)): [alpha, tau / (1 + tau)] -- the second keeps the thickness where alpha saturates."""
    alpha, tau = it.render_alpha(sub=sub, tau=True)
    return [alpha, (tau / (np.float32(1.0) + tau)).astype(np.float32)]


def film_to_xyz(film: np.ndarray) -> np.ndarray:
    """XYZ / W per pixel (main.cpp:15)."""
    return film[..., :3] / film[..., 3:4]
