"""What adaptive sampling buys on one GPU -- the measurements of EXPERIMENTS.md "Adaptive sampling".

  python tools/adaptive_ab.py [--config c3] [--reps 3] [--min 64] [--max 256] [--steps 64,32] [--percentiles 50,75,90]

The uniform frame (the config's size and spp) is timed with and without the moment plane attached; its own per-tile
errors (vpt_gpu_tile_errors) give the targets: their 50th, 75th and 90th percentile.  vpt_gpu_render_adaptive then
runs at each target and each step width, `reps` times after a warm-up, interleaved rep by rep with the one-launch
driver (vpt_gpu_render_adaptive_fused, whose waves and errors must equal the rounds driver's) and the uniform frame,
so the three legs share the session's clocks.  Every timing
is synchronised wall time around the whole driver call (it is synchronous: its rounds read the errors back), film
and plane zeroed outside it; the uniform frame is timed the same way around render_jobs + synchronize.  Best and
worst of the repetitions are reported (measuring-on-mi355x: warm up, repeat, report the spread).  Prints one JSON
line last.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def stats(v):
    return {"best_ms": round(min(v), 3), "worst_ms": round(max(v), 3), "runs_ms": [round(x, 3) for x in v]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min", type=int, default=64)
    ap.add_argument("--max", type=int, default=None, help="the cap (default: the config's spp)")
    ap.add_argument("--steps", default="64,32")
    ap.add_argument("--percentiles", default="50,75,90")
    ap.add_argument("--abs-floor", type=float, default=1e-3)
    ap.add_argument("--size", default=None, help="WxH (default: the config's)")
    args = ap.parse_args()

    import torch

    from volume_path_tracer_amd import capi
    from volume_path_tracer_amd.render import Integrator
    from volume_path_tracer_amd.scenes import SynthGrid, workload

    kw = {}
    if args.size:
        kw["width"], kw["height"] = (int(v) for v in args.size.lower().split("x"))
    wl = workload(args.config, **kw)
    dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
    temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
    it = Integrator(wl.cfg, dens, temp, device=0)
    it.tile_costs()  # (the cost pass, outside every timing)
    L = capi.lib()
    T, cap = it.jobs_per_wave, args.max or wl.spp
    film = torch.zeros_like(it.film)
    m2 = torch.zeros((wl.cfg.height, wl.cfg.width), dtype=torch.float32, device=it.dev)
    s = C.c_void_p(it.stream_handle())

    def wall(fn):
        film.zero_()
        m2.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # the uniform frame, without and with the plane (the first call of each sizes the sample buffer: dropped)
    uni = {"plain": [], "with_plane": []}
    for rep in range(args.reps + 1):
        for name in ("plain", "with_plane"):
            it.set_film_moments(m2 if name == "with_plane" else None)
            ms = wall(lambda: it.render_jobs(0, cap * T, film=film))
            if rep:
                uni[name].append(ms)
    err_u = it.tile_errors(m2, film=film, abs_floor=args.abs_floor)  # (the last frame had the plane attached)
    it.set_film_moments(None)
    launches0 = it.film_order_info()["ordered_launches"]
    out = {"what": "adaptive_ab", "config": args.config, "size": [wl.cfg.width, wl.cfg.height], "cap_waves": cap,
           "min_waves": args.min, "tiles": T, "abs_floor": args.abs_floor,
           "uniform": {k: stats(v) for k, v in uni.items()},
           "uniform_tile_error": {"max": float(err_u.max()), "mean": float(err_u.mean()),
                                  "zero_tiles": int((err_u == 0).sum())},
           "runs": []}
    waves, err = np.zeros(T, np.uint32), np.zeros(T, np.float32)
    res = capi.AdaptiveResult()
    waves_f, err_f, res_f = np.zeros(T, np.uint32), np.zeros(T, np.float32), capi.AdaptiveResult()
    has_fused = hasattr(L, "vpt_gpu_render_adaptive_fused")  # (older builds in A/B runs lack it)
    # round 0 alone (target inf: every tile stops after min_waves) -- the driver's fixed part
    p_inf = capi.AdaptiveParams(float("inf"), args.abs_floor, args.min, 64, cap)

    def round0():
        capi.check(L.vpt_gpu_render_adaptive(it.h, C.byref(p_inf), C.c_void_p(film.data_ptr()), C.c_void_p(m2.data_ptr()),
                                             waves.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             err.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res), s),
                   "vpt_gpu_render_adaptive")

    out["round0_only"] = stats([wall(round0) for _ in range(args.reps + 1)][1:])
    if has_fused:  # the fused driver's: one group of min_waves lanes per tile, every wavefront draining on its slowest lane

        def round0_fused():
            capi.check(L.vpt_gpu_render_adaptive_fused(it.h, C.byref(p_inf), C.c_void_p(film.data_ptr()),
                                                       C.c_void_p(m2.data_ptr()), waves.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                       err.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res), s),
                       "vpt_gpu_render_adaptive_fused")

        out["round0_only_fused"] = stats([wall(round0_fused) for _ in range(args.reps + 1)][1:])
    launches0 = it.film_order_info()["ordered_launches"]
    for pct in [float(x) for x in args.percentiles.split(",")]:
        target = float(np.percentile(err_u, pct))
        for step in [int(x) for x in args.steps.split(",")]:
            p = capi.AdaptiveParams(target, args.abs_floor, args.min, step, cap)

            def run(fused=False):
                name = "vpt_gpu_render_adaptive_fused" if fused else "vpt_gpu_render_adaptive"
                capi.check(getattr(L, name)(it.h, C.byref(p), C.c_void_p(film.data_ptr()), C.c_void_p(m2.data_ptr()),
                                            (waves_f if fused else waves).ctypes.data_as(C.POINTER(C.c_uint32)),
                                            (err_f if fused else err).ctypes.data_as(C.POINTER(C.c_float)),
                                            C.byref(res_f if fused else res), s), name)

            # one warm-up of each leg (dropped), then the legs interleaved rep by rep: fused, rounds, uniform
            wall(run)
            n_launch = it.film_order_info()["ordered_launches"] - launches0
            ms, ms_f, ms_u = [], [], []
            if has_fused:
                wall(lambda: run(True))
            for _ in range(args.reps):
                if has_fused:
                    ms_f.append(wall(lambda: run(True)))
                    film_f = film.clone()
                ms.append(wall(run))
                if has_fused:  # the same frame, or the comparison means nothing
                    assert waves_f.tobytes() == waves.tobytes() and err_f.tobytes() == err.tobytes()
                    assert torch.equal(film_f, film) and res_f.rounds == res.rounds
                ms_u.append(wall(lambda: it.render_jobs(0, cap * T, film=film)))
            launches0 = it.film_order_info()["ordered_launches"]
            vals, counts = np.unique(waves, return_counts=True)
            # Where the time goes: the tiles that reached the cap, all their waves as ONE list launch (what their
            # work costs when it is not cut into rounds), and the launch of one later round alone (the first
            # step_waves waves after round 0 of those tiles).
            at_cap = np.flatnonzero(waves == cap).astype(np.uint32)
            extra = {}
            if at_cap.size:
                one = [wall(lambda: it.render_tile_list(at_cap, 1, cap, film=film)) for _ in range(2)][1:]
                rnd = [wall(lambda: it.render_tile_list(at_cap, args.min + 1, step, film=film)) for _ in range(2)][1:]
                extra = {"capped_tiles_all_waves_one_launch_ms": round(min(one), 3),
                         "capped_tiles_one_round_launch_ms": round(min(rnd), 3)}
                launches0 = it.film_order_info()["ordered_launches"]
            out["runs"].append({"percentile": pct, "target": target, "step_waves": step, **stats(ms), **extra,
                                "jobs_ratio": round(res.jobs_rendered / res.jobs_uniform, 4), "rounds": int(res.rounds),
                                "launches_per_frame": n_launch,
                                "fused": stats(ms_f) if has_fused else None, "uniform_interleaved": stats(ms_u),
                                "fused_vs_rounds": round(min(ms_f) / min(ms), 4) if has_fused else None,
                                "fused_vs_uniform": round(min(ms_f) / min(ms_u), 4) if has_fused else None,
                                "waves_histogram": {int(v): int(c) for v, c in zip(vals, counts)},
                                "tile_error": {"max": float(err.max()), "mean": float(err.mean())},
                                "vs_uniform_plain": round(min(ms) / min(uni["plain"]), 4)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
