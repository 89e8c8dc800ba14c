"""What the depth pass costs beside the matte and a frame -- the measurements of EXPERIMENTS.md §25.

  python tools/depth_ab.py [--config c3] [--opacity 0.00392157,0.5] [--sub 1] [--reps 5] [--size WxH] [--spp N]

Times vpt_gpu_render_depth (the C-ABI call on caller-owned planes, so no allocation or read-back is inside a timing) at
the given levels and sub-ray count with HIP events on the context's stream, `reps` times after a warm-up call,
interleaved rep by rep with vpt_gpu_render_alpha at the same sub-ray count and with the config's uniform frame
(render_jobs of all its waves, timed the same way), so all three share the session's clocks.  Reports best and worst of
the repetitions (measuring-on-mi355x: warm up, repeat, report the spread), how many pixels reach each level, and checks
that depth > 0 exactly where the matte's tau plane reaches the level (sub = 1).  Prints one JSON line last.
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
    ap.add_argument("--opacity", default="0.00392157,0.5")
    ap.add_argument("--sub", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", default=None, help="WxH (default: the config's)")
    ap.add_argument("--spp", type=int, default=None, help="the uniform frame's waves (default: the config's)")
    args = ap.parse_args()

    import numpy as np
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
    op = np.ascontiguousarray([float(v) for v in args.opacity.split(",")], np.float32)
    film = torch.zeros_like(it.film)
    alpha = torch.zeros((wl.cfg.height, wl.cfg.width), dtype=torch.float32, device=it.dev)
    tau = torch.zeros_like(alpha)
    depth = torch.zeros((op.size, wl.cfg.height, wl.cfg.width), dtype=torch.float32, device=it.dev)
    reach = torch.zeros_like(depth)
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

    def matte():
        capi.check(L.vpt_gpu_render_alpha(it.h, args.sub, C.c_void_p(alpha.data_ptr()), C.c_void_p(tau.data_ptr()), s),
                   "vpt_gpu_render_alpha")

    def planes():
        capi.check(L.vpt_gpu_render_depth(it.h, args.sub, op.size, op.ctypes.data_as(C.POINTER(C.c_float)),
                                          C.c_void_p(depth.data_ptr()), C.c_void_p(reach.data_ptr()), s),
                   "vpt_gpu_render_depth")

    out = {"config": args.config, "size": [wl.cfg.width, wl.cfg.height], "spp": wl.spp, "grid_n": wl.grid_n,
           "reps": args.reps, "sub": args.sub, "opacity": [float(a) for a in op], "frame": [], "alpha": [], "depth": []}
    for rep in range(args.reps + 1):  # (rep 0 warms up: the frame's first call sizes the sample buffer)
        for name, fn in (("frame", frame), ("alpha", matte), ("depth", planes)):
            ms = timed(fn)
            if rep:
                out[name].append(ms)
    for name in ("frame", "alpha", "depth"):
        out[name] = stats(out[name])
    out["depth"]["of_alpha"] = round(out["depth"]["best_ms"] / out["alpha"]["best_ms"], 4)
    out["depth"]["of_frame"] = round(out["depth"]["best_ms"] / out["frame"]["best_ms"], 5)
    d, t = depth.cpu().numpy(), tau.cpu().numpy()
    out["reached_pixels"] = [float((d[k] > 0).mean()) for k in range(op.size)]
    if args.sub == 1 or not wl.cfg.worker_parameters.use_jitter:
        tk = (-np.log1p(-op.astype(np.float64))).astype(np.float32)
        out["reach_equals_tau_plane"] = bool(all(np.array_equal(d[k] > 0, t >= tk[k]) for k in range(op.size)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
