"""Band launches (vpt_gpu_render_tiles) against job-range launches (vpt_gpu_render_jobs) on one GPU, one binary,
one context -- the measurements of EXPERIMENTS.md "Tile-band launches".  A and B alternate inside one process
(measuring-on-mi355x: interleave, report best-of and spread); every timing is a pair of HIP events around one call.

  python tools/band_ab.py frame  [--config c3] [--reps 5]      whole frame: render_jobs vs render_tiles(0, T)
  python tools/band_ab.py shares [--config c3] [--reps 3] [--gpus 2,4,8]
        emulated strong scaling: every rank's share timed alone on this GPU, the slowest band share
        (distributed.cost_bands) against the slowest wave share (rank_job_ranges "strong")
  python tools/band_ab.py one --kind jobs|tiles [--config c3]  one launch, nothing else (under rocprofv3 --pmc)
  python tools/band_ab.py pmc <dir>...                         per-kernel counter sums of such runs
Each prints one JSON line last.  tools/band_ab.sh runs them all with time limits.
"""
from __future__ import annotations

import argparse
import csv
import json
import sys
from collections import defaultdict
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def make(config):
    import torch

    from volume_path_tracer_amd.render import Integrator
    from volume_path_tracer_amd.scenes import SynthGrid, workload

    wl = workload(config)
    dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
    temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
    it = Integrator(wl.cfg, dens, temp, device=0)
    it.tile_costs()  # (the cost pass, outside every timing)
    return torch, wl, it


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


def cmd_frame(args):
    torch, wl, it = make(args.config)
    T, spp = it.jobs_per_wave, wl.spp
    film = torch.zeros_like(it.film)
    jobs = lambda: it.render_jobs(0, spp * T, film=film)  # noqa: E731
    tiles = lambda: it.render_tiles(0, T, 1, spp, film=film)  # noqa: E731
    films = {}
    for name, fn in (("jobs", jobs), ("tiles", tiles)):  # warm-up (sizes the sample buffer) and the films
        film.zero_()
        timed(torch, fn)
        films[name] = film.cpu().numpy().tobytes()
    t = {"jobs": [], "tiles": []}
    for _ in range(args.reps):
        for name, fn in (("jobs", jobs), ("tiles", tiles)):
            t[name].append(timed(torch, fn))
    out = {"what": "frame", "config": args.config, "spp": spp, "tiles": T, "films_equal": films["jobs"] == films["tiles"],
           "render_jobs": stats(t["jobs"]), "render_tiles": stats(t["tiles"]), "film_order": it.film_order_info()}
    print(json.dumps(out))


def cmd_shares(args):
    from volume_path_tracer_amd import distributed as D

    torch, wl, it = make(args.config)
    T, spp = it.jobs_per_wave, wl.spp
    cost, _ = it.tile_costs()
    film = torch.zeros_like(it.film)
    # the largest launches first, so the sample buffer never grows inside a timing
    timed(torch, lambda: it.render_tiles(0, T, 1, spp, film=film))
    out = {"what": "shares", "config": args.config, "spp": spp, "tiles": T, "gpus": {}}
    for n in [int(x) for x in args.gpus.split(",")]:
        cut = D.cost_bands(cost, n)
        wave = [[] for _ in range(n)]
        band = [[] for _ in range(n)]
        for rep in range(args.reps + 1):  # (rep 0: warm-up, dropped)
            for r in range(n):
                tw = 0.0
                for b, c in D.rank_job_ranges(r, n, spp, T, "strong"):
                    tw += timed(torch, lambda: it.render_jobs(b, c, film=film))
                tb = timed(torch, lambda: it.render_tiles(cut[r], cut[r + 1], 1, spp, film=film))
                if rep:
                    wave[r].append(tw)
                    band[r].append(tb)
        slow_w = max(min(v) for v in wave)
        slow_b = max(min(v) for v in band)
        out["gpus"][str(n)] = {"cuts": cut, "wave_share_best_ms": [round(min(v), 3) for v in wave],
                               "band_share_best_ms": [round(min(v), 3) for v in band],
                               "wave_share_spread_ms": [round(max(v) - min(v), 3) for v in wave],
                               "band_share_spread_ms": [round(max(v) - min(v), 3) for v in band],
                               "slowest_wave_share_ms": round(slow_w, 3), "slowest_band_share_ms": round(slow_b, 3)}
    print(json.dumps(out))


def cmd_one(args):
    torch, wl, it = make(args.config)
    T, spp = it.jobs_per_wave, wl.spp
    if args.kind == "jobs":
        ms = timed(torch, lambda: it.render_jobs(0, spp * T))
    else:
        ms = timed(torch, lambda: it.render_tiles(0, T, 1, spp))
    print(json.dumps({"what": "one", "kind": args.kind, "config": args.config, "ms_under_profiler": round(ms, 3)}))


def cmd_pmc(args):
    kernels = ("vpt_integrate_kernel", "vpt_film_order_kernel", "vpt_band_order_kernel")
    per = defaultdict(float)
    for d in args.dirs:
        for f in Path(d).rglob("*counter_collection.csv"):
            for r in csv.DictReader(open(f)):
                k = next((k for k in kernels if k in r["Kernel_Name"]), None)
                if k:
                    per[(k, r["Counter_Name"])] += float(r["Counter_Value"])
    out = defaultdict(dict)
    for (k, c), v in sorted(per.items()):
        out[k][c] = v
    for k, c in out.items():
        if "TCC_EA0_WRREQ_sum" in c and "TCC_EA0_WRREQ_64B_sum" in c:
            c["wrreq_32B"] = c["TCC_EA0_WRREQ_sum"] - c["TCC_EA0_WRREQ_64B_sum"]
        if "WRITE_SIZE" in c:
            c["write_bytes"] = c["WRITE_SIZE"] * 1024
    print(json.dumps({"what": "pmc", "dirs": args.dirs, "kernels": out}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("frame", "shares", "one"):
        p = sub.add_parser(name)
        p.add_argument("--config", default="c3")
        p.add_argument("--reps", type=int, default=5 if name == "frame" else 3)
        if name == "shares":
            p.add_argument("--gpus", default="2,4,8")
        if name == "one":
            p.add_argument("--kind", choices=("jobs", "tiles"), required=True)
    p = sub.add_parser("pmc")
    p.add_argument("dirs", nargs="+")
    args = ap.parse_args()
    {"frame": cmd_frame, "shares": cmd_shares, "one": cmd_one, "pmc": cmd_pmc}[args.cmd](args)


if __name__ == "__main__":
    main()
