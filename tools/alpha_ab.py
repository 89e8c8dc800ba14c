"""What the coverage pass costs beside a frame -- the measurements of EXPERIMENTS.md §17.

  python tools/alpha_ab.py [--config c3] [--subs 1,4] [--reps 5] [--size WxH] [--spp N]

Times vpt_gpu_render_alpha (Integrator's C-ABI call on caller-owned planes, so no allocation or read-back is inside a
timing) at each sub-ray count with HIP events on the context's stream, `reps` times after a warm-up call, interleaved
rep by rep with the config's uniform frame (render_jobs of all its waves, timed the same way), so both share the
session's clocks.  Reports best and worst of the repetitions (measuring-on-mi355x: warm up, repeat, report the
spread), the matte's coverage statistics, and the HDDA steps per primary ray of the frame for scale.  Prints one JSON
line last.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def stats(v):
    return {"best_ms": round(min(v), 3), "worst_ms": round(max(v), 3), "runs_ms": [round(x, 3) for x in v]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c3")
    ap.add_argument("--subs", default="1,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", default=None, help="WxH (default: the config's)")
    ap.add_argument("--spp", type=int, default=None, help="the uniform frame's waves (default: the config's)")
    args = ap.parse_args()

    import torch

    from volume_path_tracer_amd import capi
    from volume_path_tracer_amd.render import Integrator
    from volume_path_tracer_amd.scenes import SynthGrid, workload

    kw = {}
    if args.size:
        kw["width"], kw["height"] = (int(v) for v in args.size.lower().split("x"))
    if args.spp:
        kw["spp"] = args.spp
    wl = workload(args.config, **kw)
    dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
    temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
    it = Integrator(wl.cfg, dens, temp, device=0)
    it.tile_costs()  # (the cost pass, outside every timing)
    L = capi.lib()
    subs = [int(v) for v in args.subs.split(",")]
    film = torch.zeros_like(it.film)
    alpha = torch.zeros((wl.cfg.height, wl.cfg.width), dtype=torch.float32, device=it.dev)
    tau = torch.zeros_like(alpha)
    s = C.c_void_p(it.stream_handle())

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def frame():
        film.zero_()
        it.render_jobs(0, wl.spp * it.jobs_per_wave, film=film)

    def matte(sub):
        capi.check(L.vpt_gpu_render_alpha(it.h, sub, C.c_void_p(alpha.data_ptr()), C.c_void_p(tau.data_ptr()), s),
                   "vpt_gpu_render_alpha")

    out = {"config": args.config, "size": [wl.cfg.width, wl.cfg.height], "spp": wl.spp, "grid_n": wl.grid_n,
           "reps": args.reps, "frame": [], "alpha": {str(k): [] for k in subs}}
    for rep in range(args.reps + 1):  # (rep 0 warms up: the frame's first call sizes the sample buffer)
        ms = timed(frame)
        if rep:
            out["frame"].append(ms)
        for k in subs:
            ms = timed(lambda: matte(k))
            if rep:
                out["alpha"][str(k)].append(ms)
    out["frame"] = stats(out["frame"])
    out["alpha"] = {k: stats(v) for k, v in out["alpha"].items()}
    for k in subs:
        out["alpha"][str(k)]["of_frame"] = round(out["alpha"][str(k)]["best_ms"] / out["frame"]["best_ms"], 4)
    a = alpha.cpu().numpy()
    t = tau.cpu().numpy()
    out["coverage"] = {"covered_pixels": float((a > 0).mean()), "mean_alpha": float(a.mean()), "max_tau": float(t.max())}
    c = it.counters()
    if c.get("samples"):
        out["frame_dda_steps_per_sample"] = round(c["dda_steps"] / c["samples"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
