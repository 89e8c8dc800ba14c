"""The stencil pool's two layouts (vpt_gpu_set_pool_layout) on one GPU, one binary, one context -- the switch
measurement of EXPERIMENTS.md "Direct-addressed stencil pool".  VPT_POOL_SPARSE and VPT_POOL_DENSE alternate inside
one process (measuring-on-mi355x: interleave, report best-of and spread), so the kernel's code is the same on both
sides and the difference is the layout's alone; every timing is a pair of HIP events around one whole-frame launch,
the switch (free / allocate / expand) outside it.

  python tools/pool_ab.py [--config c3] [--pairs 5]

Prints one JSON line last: the frame times per layout, whether the films are the same bytes, both pools' bytes and
the expansion kernels' time.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {"best_ms": round(min(v), 3), "worst_ms": round(max(v), 3), "runs_ms": [round(x, 3) for x in v]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c3")
    ap.add_argument("--pairs", type=int, default=5)
    args = ap.parse_args()
    import torch

    from volume_path_tracer_amd import capi
    from volume_path_tracer_amd.render import Integrator
    from volume_path_tracer_amd.scenes import SynthGrid, workload

    wl = workload(args.config)
    dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
    temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
    it = Integrator(wl.cfg, dens, temp, device=0)
    it.tile_costs()  # (the cost pass, outside every timing)
    jobs = wl.spp * it.jobs_per_wave
    film = torch.zeros_like(it.film)
    layouts = (("sparse", capi.VPT_POOL_SPARSE), ("dense", capi.VPT_POOL_DENSE))
    films, info, t = {}, {}, {"sparse": [], "dense": []}
    for name, layout in layouts:  # warm-up (sizes the sample buffer) and the films
        it.set_pool_layout(layout)
        info[name] = it.pool_info()
        film.zero_()
        timed(torch, lambda: it.render_jobs(0, jobs, film=film))
        films[name] = film.cpu().numpy().tobytes()
    for _ in range(args.pairs):
        for name, layout in layouts:
            it.set_pool_layout(layout)
            t[name].append(timed(torch, lambda: it.render_jobs(0, jobs, film=film)))
    print(json.dumps({"what": "pool_ab", "config": args.config, "spp": wl.spp, "films_equal": films["sparse"] == films["dense"],
                      "sparse": stats(t["sparse"]), "dense": stats(t["dense"]),
                      "dense_bytes": info["dense"]["dense_bytes"], "sparse_bytes": info["dense"]["sparse_bytes"],
                      "expand_ms": round(info["dense"]["expand_ms"], 3)}))


if __name__ == "__main__":
    main()
