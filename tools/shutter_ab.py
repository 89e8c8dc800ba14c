"""What the shutter costs -- the measurements of EXPERIMENTS.md section 24.

  bash tools/build_rev_lib.sh <parent commit> parent          # volume_path_tracer_amd/lib/libvpt_parent.so
  python tools/shutter_ab.py [--configs c3,c4] [--rounds 5] [--frames 2] [--size WxH] [--spp N] [--grid-n N]
                             [--entries 256] [--parent-lib PATH]

Three sides of the config's one-launch frame (render_jobs of all its waves):
  (a) the parent commit's library;
  (b) this tree's with nothing attached -- the bar: its range overlaps (a)'s (the kernels a plain launch runs are the
      parent's, DESIGN.md section 15's resource table; this run confirms it);
  (c) this tree's with a shutter of `entries` cameras, all of them the scene's camera: the same rays, the same film
      bytes (checked), so the difference to (b) is the per-lane camera loads and the Shutter kernels alone.
`rounds` times a fresh process per library (VPT_LIB), alternating, each under its own time limit, each one warm-up frame
and `frames` timed ones per side with HIP events on the context's stream; (b) and (c) share a process.  Reports best and
worst of all repetitions (measuring-on-mi355x: warm up, repeat, alternate, report the spread).  Prints one JSON line
last.
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

    res = {"config": args.child, "lib": os.environ.get("VPT_LIB", "tree"), "plain_ms": frames(args.frames)}
    plain_bytes = film.cpu().numpy().tobytes()
    if hasattr(capi.lib(), "vpt_gpu_set_shutter"):
        it.set_shutter([{}] * args.entries)
        res["shutter_ms"] = frames(args.frames)
        res["film_same_bytes"] = film.cpu().numpy().tobytes() == plain_bytes
        it.set_shutter(None)
    print("SH_AB " + json.dumps(res), flush=True)


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
    ap.add_argument("--entries", type=int, default=256)
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
                cmd = [sys.executable, "-B", __file__, "--child", cfg, "--frames", str(args.frames), "--entries",
                       str(args.entries)]
                for flag, v in (("--size", args.size), ("--spp", args.spp), ("--grid-n", args.grid_n)):
                    if v:
                        cmd += [flag, str(v)]
                # a fresh process per library, one at a time, each under its own time limit; a step that fails ends the run
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("SH_AB ")]
                if p.returncode != 0 or not line:
                    sys.exit(f"{cfg} {side} round {r}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
                runs[side].append(json.loads(line[-1][6:]))
                print(f"{cfg} round {r} {side}: {runs[side][-1]}", file=sys.stderr, flush=True)
        flat = lambda side, key: [x for c in runs[side] for x in c.get(key, [])]  # noqa: E731
        pa, tr, sh = flat("parent", "plain_ms"), flat("tree", "plain_ms"), flat("tree", "shutter_ms")
        out[cfg] = {"a_parent": spread(pa), "b_tree_plain": spread(tr), "c_tree_shutter": spread(sh),
                    "b_overlaps_a": min(tr) <= max(pa) and min(pa) <= max(tr),
                    # each process's shuttered frames against its own plain frames
                    "c_over_b": [round(min(c["shutter_ms"]) / min(c["plain_ms"]), 4) for c in runs["tree"]],
                    "entries": args.entries,
                    "film_same_bytes": all(c["film_same_bytes"] for c in runs["tree"])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
