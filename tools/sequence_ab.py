"""What one context per sequence saves -- the measurements of EXPERIMENTS.md "Sequences".

  python tools/sequence_ab.py [--configs c3,c4] [--frames 8] [--size WxH] [--spp N] [--grid N]

For each config (its size, spp and 512^3 stand-in unless overridden) an orbit of `frames` cameras is rendered twice in
one process: (a) a new Integrator per frame, the only way before vpt_gpu_set_scene and the baseline; (b) one
Integrator moved by set_scene.  Per frame: the update (a: destroy + create; b: set_scene), the tile-cost pass (the
increase of setup_timings()' tile_costs entry over the frame), the launch (render_jobs + synchronize, the cost pass
taken out) and the wall time of the whole frame.  The grids are generated and described once, outside every timing;
(a) still flattens and uploads them per frame, as a caller without the update must.  The films of (a) and (b) must
be the same bytes, frame by frame.

Then the volume swap: between two equal-sized stand-ins (the config's density and the same lattice negated in one
slab), set_volume + set_scene against destroy + create, `frames` times alternating.

Frame 0 of both legs pays the first launch's one-time costs; the ranges are reported over frames 1.. (measuring on
a shared machine: warm up, repeat, report the spread).  The one defect this tool looks for: (b)'s launch time of a
frame outside (a)'s launch times of the same camera by more than (a)'s own frame-to-frame spread -- a stale tile
order.  Prints one JSON line last.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def span(v):
    return {"min_ms": round(min(v), 2), "max_ms": round(max(v), 2)} if v else {}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="c3,c4")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default=None, help="WxH (default: the config's)")
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--grid", type=int, default=None, help="lattice size (default: the config's, 512)")
    args = ap.parse_args()

    import torch

    from volume_path_tracer_amd import capi
    from volume_path_tracer_amd.render import Integrator
    from volume_path_tracer_amd.scenes import SynthGrid, orbit, workload

    kw = {"spp": args.spp, "grid_n": args.grid}
    if args.size:
        kw["width"], kw["height"] = (int(v) for v in args.size.lower().split("x"))
    out = {}
    for name in args.configs.split(","):
        wl = workload(name, **kw)
        dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
        temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
        cfgs = orbit(wl.cfg, args.frames)
        film = None

        def frame(it):
            """One frame from zero -> (launch ms with the cost pass taken out, cost pass ms, film bytes)."""
            nonlocal film
            if film is None:
                film = torch.zeros_like(it.film)
            film.zero_()
            torch.cuda.synchronize()
            c0 = it.setup_timings()["tile_costs"]
            t0 = time.perf_counter()
            it.render_jobs(0, it.total_jobs, film=film)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            cost = it.setup_timings()["tile_costs"] - c0
            return ms - cost, cost, film.cpu().numpy().tobytes()

        legs = {"fresh": [], "set_scene": []}
        films = {"fresh": [], "set_scene": []}
        it = None
        for c in cfgs:  # (a) a context per frame
            t0 = time.perf_counter()
            it = None  # (destroy: the previous frame's context goes before the next is created, as a caller would)
            it = Integrator(c, dens, temp, device=0)
            torch.cuda.synchronize()
            upd = (time.perf_counter() - t0) * 1e3
            launch, cost, fb = frame(it)
            legs["fresh"].append({"update_ms": upd, "cost_ms": cost, "launch_ms": launch,
                                  "wall_ms": (time.perf_counter() - t0) * 1e3, "setup": it.setup_timings()})
            films["fresh"].append(fb)
        it = None
        it = Integrator(cfgs[0], dens, temp, device=0)
        for k, c in enumerate(cfgs):  # (b) one context
            t0 = time.perf_counter()
            if k:
                it.set_scene(c)
            upd = (time.perf_counter() - t0) * 1e3
            launch, cost, fb = frame(it)
            legs["set_scene"].append({"update_ms": upd, "cost_ms": cost, "launch_ms": launch,
                                      "wall_ms": (time.perf_counter() - t0) * 1e3})
            films["set_scene"].append(fb)
        same = films["fresh"] == films["set_scene"]
        distinct = len(set(films["fresh"])) == len(cfgs)
        res = {"frames": len(cfgs), "size": [wl.cfg.width, wl.cfg.height], "spp": wl.spp, "grid": wl.grid_n,
               "films_equal": same, "frames_distinct": distinct}
        for leg, rows in legs.items():
            res[leg] = {k: span([r[k] for r in rows[1:]]) for k in ("update_ms", "cost_ms", "launch_ms", "wall_ms")}
            res[leg]["per_frame"] = [{k: round(v, 2) for k, v in r.items() if k != "setup"} for r in rows]
        res["fresh"]["setup_last"] = {k: round(v, 2) for k, v in legs["fresh"][-1]["setup"].items()}
        # the defect: a launch after set_scene slower than the fresh context's for that camera by more than the fresh
        # leg's own spread
        spread = res["fresh"]["launch_ms"]["max_ms"] - res["fresh"]["launch_ms"]["min_ms"] if len(cfgs) > 1 else 0.0
        res["launch_excess_ms"] = [round(b["launch_ms"] - a["launch_ms"], 2)
                                   for a, b in zip(legs["fresh"][1:], legs["set_scene"][1:])]
        res["fresh_launch_spread_ms"] = round(spread, 2)

        # the volume swap between two equal-sized volumes
        other = capi.Grid.from_desc(dens.desc, copy=True)
        slab = other.leaf_origin[:, 0] < wl.grid_n // 2
        other.leaf_values[slab] *= np.float32(0.5)
        other.leaf_max[:] = other.leaf_values.max(axis=1)
        vols = [dens, other]
        swap = {"fresh": [], "set_volume": []}
        sf = {"fresh": [], "set_volume": []}
        for k in range(args.frames):
            t0 = time.perf_counter()
            it = None
            it = Integrator(cfgs[0], vols[k % 2], temp, device=0)
            torch.cuda.synchronize()
            upd = (time.perf_counter() - t0) * 1e3
            launch, cost, fb = frame(it)
            swap["fresh"].append({"update_ms": upd, "cost_ms": cost, "launch_ms": launch})
            sf["fresh"].append(fb)
        for k in range(args.frames):
            t0 = time.perf_counter()
            if k:
                it.set_volume(vols[k % 2], temp)
                it.set_scene(cfgs[0])
            upd = (time.perf_counter() - t0) * 1e3
            launch, cost, fb = frame(it)
            swap["set_volume"].append({"update_ms": upd, "cost_ms": cost, "launch_ms": launch})
            sf["set_volume"].append(fb)
        # (the swapped context is the last fresh one: its frame 0 renders that context's volume)
        res["swap"] = {"films_equal": all(sf["set_volume"][k] == sf["fresh"][k if k else args.frames - 1]
                                          for k in range(args.frames)),
                       "volumes_distinct": sf["fresh"][0] != sf["fresh"][1] if args.frames > 1 else None}
        for leg, rows in swap.items():
            res["swap"][leg] = {k: span([r[k] for r in rows[1:]]) for k in ("update_ms", "cost_ms", "launch_ms")}
        it = None
        film = None
        out[name] = res
        print(f"{name}: fresh update {res['fresh']['update_ms']} launch {res['fresh']['launch_ms']}; set_scene update "
              f"{res['set_scene']['update_ms']} cost pass {res['set_scene']['cost_ms']} launch "
              f"{res['set_scene']['launch_ms']}; films equal {same}; swap fresh {res['swap']['fresh']['update_ms']} "
              f"set_volume {res['swap']['set_volume']['update_ms']} equal {res['swap']['films_equal']}", file=sys.stderr)
    print(json.dumps({"sequence_ab": out}))


if __name__ == "__main__":
    main()
