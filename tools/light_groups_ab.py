"""What light groups cost -- the measurements of EXPERIMENTS.md section 23.

  bash tools/build_rev_lib.sh <parent commit> parent          # volume_path_tracer_amd/lib/libvpt_parent.so
  python tools/light_groups_ab.py [--configs c3,c4] [--rounds 5] [--frames 2] [--size WxH] [--spp N] [--grid-n N]
                                  [--parent-lib PATH]

Off-cost.  The config's one-launch frame (render_jobs of all its waves, nothing attached) with the parent commit's
library and with this tree's, alternating: `rounds` times a fresh process per library (VPT_LIB), each one warm-up frame
and `frames` timed ones with HIP events on the context's stream.  The bar: the two ranges overlap (the kernels a plain
launch runs are the parent's, DESIGN.md section 14's resource table; this run confirms it).

On-cost.  In this tree's processes, after the plain frames: the same frame with group planes attached (one warm-up,
`frames` timed), against that process's plain frames; the sample buffer's bytes of both.

Relight.  One vpt_gpu_relight at the frame's size: 20 calls after a warm-up, HIP events around each.

Reports best and worst of all repetitions (measuring-on-mi355x: warm up, repeat, alternate, report the spread).  Prints
one JSON line last.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def child(args) -> None:
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
    if args.grid_n:
        kw["grid_n"] = args.grid_n
    wl = workload(args.child, **kw)
    dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
    temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
    it = Integrator(wl.cfg, dens, temp, device=0)
    jobs = wl.cfg.jobs_per_wave() * wl.spp
    film = torch.zeros_like(it.film)

    def frames(n):
        out = []
        for k in range(n + 1):  # (the first is the warm-up)
            film.zero_()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            it.render_jobs(0, jobs, film=film)
            b.record()
            b.synchronize()
            if k:
                out.append(a.elapsed_time(b))
        return out

    res = {"config": args.child, "lib": os.environ.get("VPT_LIB", "tree"), "plain_ms": frames(args.frames),
           "plain_buffer_bytes": it.film_order_info()["buffer_bytes"]}
    plain_bytes = film.cpu().numpy().tobytes()
    if hasattr(capi.lib(), "vpt_gpu_set_light_groups"):
        gp = torch.zeros((3, wl.cfg.height, wl.cfg.width, 4), dtype=torch.float32, device=it.dev)
        it.set_light_groups(gp)
        res["groups_ms"] = frames(args.frames)
        res["groups_buffer_bytes"] = it.film_order_info()["buffer_bytes"]
        res["film_same_bytes"] = film.cpu().numpy().tobytes() == plain_bytes
        it.set_light_groups(None)
        k = np.array([[1.5, 1.25, 0.75], [0.5, 2.0, 3.0], [0.3, 0.7, 1.1]], np.float32)
        ms = []
        for i in range(21):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            it.relight(gp, k)
            b.record()
            b.synchronize()
            if i:
                ms.append(a.elapsed_time(b))
        res["relight_ms"] = ms
    print("LG_AB " + json.dumps(res), flush=True)


def spread(v):
    return {"best_ms": round(min(v), 3), "worst_ms": round(max(v), 3), "n": len(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="c3,c4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--size", default=None)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--grid-n", type=int, default=None)
    ap.add_argument("--parent-lib", default=str(ROOT / "volume_path_tracer_amd" / "lib" / "libvpt_parent.so"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not Path(args.parent_lib).exists():
        sys.exit(f"{args.parent_lib}: build it first (bash tools/build_rev_lib.sh <parent commit> parent)")
    out = {}
    for cfg in args.configs.split(","):
        runs = {"parent": [], "tree": []}
        for r in range(args.rounds):
            for side in ("parent", "tree"):
                env = dict(os.environ)
                env.pop("VPT_LIB", None)
                if side == "parent":
                    env["VPT_LIB"] = args.parent_lib
                cmd = [sys.executable, "-B", __file__, "--child", cfg, "--frames", str(args.frames)]
                for flag, v in (("--size", args.size), ("--spp", args.spp), ("--grid-n", args.grid_n)):
                    if v:
                        cmd += [flag, str(v)]
                # a fresh process per library, one at a time, each under its own time limit
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("LG_AB ")]
                if p.returncode != 0 or not line:
                    sys.exit(f"{cfg} {side} round {r}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
                runs[side].append(json.loads(line[-1][6:]))
                print(f"{cfg} round {r} {side}: {runs[side][-1]}", file=sys.stderr, flush=True)
        flat = lambda side, key: [x for c in runs[side] for x in c.get(key, [])]  # noqa: E731
        pa, tr, gr = flat("parent", "plain_ms"), flat("tree", "plain_ms"), flat("tree", "groups_ms")
        rec = {"parent_plain": spread(pa), "tree_plain": spread(tr), "tree_groups": spread(gr),
               "off_cost_ranges_overlap": min(tr) <= max(pa) and min(pa) <= max(tr),
               # each process's attached frames against its own plain frames
               "on_cost_ratio": [round(min(c["groups_ms"]) / min(c["plain_ms"]), 4) for c in runs["tree"]],
               "plain_buffer_bytes": runs["tree"][0]["plain_buffer_bytes"],
               "groups_buffer_bytes": runs["tree"][0]["groups_buffer_bytes"],
               "film_same_bytes": all(c["film_same_bytes"] for c in runs["tree"]),
               "relight": spread(flat("tree", "relight_ms"))}
        out[cfg] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
